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
 * Only __ballot, __shfl, __shfl_up, __shfl_xor, __syncthreads and atomicMax / atomicOr on 32-bit LDS words: the file compiles unmodified on tests/emu/hipemu.
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
#define CRX_SEG_OUT 4640u             /* bytes a segment's output can take: 3 + 9 * CRX_SEG + 7 + 3 bits, padded to a byte, + 4: 4614, rounded up to a multiple of 32 */
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
/* length 3 .. 258, distance 1 .. 32768: at most 8 + 5 + 5 + 13 = 31 bits */
__host__ __device__ __forceinline__ void zipMatch(uint32_t length, uint32_t distance, uint64_t &code, uint32_t &bits) {
	const uint32_t l = length - 3u;
	uint32_t sym, e = 0u, x = 0u;
	if (length == 258u) sym = 285u;
	else if (l < 8u) sym = 257u + l;
	else { e = zipLog2(l) - 2u; sym = 261u + 4u * e + ((l >> e) - 4u); x = l & ((1u << e) - 1u); }
	uint32_t n;
	if (sym < 280u) { code = zipRev(sym - 256u, 7u); n = 7u; }
	else { code = zipRev(0xc0u + sym - 280u, 8u); n = 8u; }
	code |= (uint64_t)x << n; n += e;
	const uint32_t dd = distance - 1u;
	uint32_t dc = dd, de = 0u, dx = 0u;
	if (dd >= 4u) { de = zipLog2(dd) - 1u; dc = 2u * de + 2u + ((dd >> de) & 1u); dx = dd & ((1u << de) - 1u); }
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

/* One wave per segment. segOut: CRX_SEG_OUT bytes a segment; segMeta: {bytes, sum of the bytes mod 65521, sum of (len - p) * byte[p] mod 65521, 0} a segment */
__global__ __launch_bounds__(64) void k_zip_deflate(const ZipGeom G, const uint32_t *T, uint32_t *segOut, uint32_t *segMeta) {
	__shared__ uint32_t sData[CRX_SEG / 4u + 4u];
	__shared__ uint32_t sHash[1u << CRX_HASH_BITS];         /* position + 1 of the last occurrence in an earlier step, 0: none */
	__shared__ uint32_t sBits[CRX_SEG_OUT / 4u];
	const uint32_t k = blockIdx.x / G.segsPerChunk, seg = blockIdx.x - k * G.segsPerChunk;
	const uint32_t n = zipChunkBytes(G, k), begin = seg * CRX_SEG;
	if (begin >= n) return;          /* (the whole wave: a short last chunk has fewer segments) */
	const uint32_t len = zipMin(CRX_SEG, n - begin), lane = threadIdx.x;
	const bool last = begin + len == n;
	const uint32_t *const src = T + (size_t)k * G.pitch + begin / 4u;
	for (uint32_t i = lane; i < CRX_SEG / 4u + 4u; i += 64u) sData[i] = 4u * i < len ? src[i] : 0u;
	for (uint32_t i = lane; i < (1u << CRX_HASH_BITS); i += 64u) sHash[i] = 0u;
	for (uint32_t i = lane; i < CRX_SEG_OUT / 4u; i += 64u) sBits[i] = lane == 0u && i == 0u ? (last ? 1u : 0u) | 2u : 0u;          /* BFINAL, BTYPE 01 */
	__syncthreads();

	uint32_t sumA = 0u, sumB = 0u;          /* (sumB over the segment <= 255 * 4096 * 4097 / 2 < 2^31) */
	uint32_t next = 0u;                     /* where the next token starts: the greedy parse, wave-uniform */
	uint32_t at = 3u;                       /* bits written so far, wave-uniform */
	for (uint32_t step = 0; step < CRX_SEG / 64u; ++step) {
		const uint32_t base = 64u * step, p = base + lane;
		const uint32_t most = p < len ? zipMin(CRX_MAX_MATCH, len - p) : 0u;
		uint32_t h = 0u, seen = 0u, byte = 0u;
		if (p < len) {
			const uint32_t four = zipLoad4(sData, p);
			byte = four & 255u;
			sumA += byte; sumB += (len - p) * byte;
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
		/* the tokens' codes, each behind those of the lanes below */
		uint64_t code = 0u;
		uint32_t bits = 0u;
		if (token) {
			if (best) zipMatch(best, bestDistance, code, bits);
			else zipLiteral(byte, code, bits);
		}
		uint32_t sum = bits;
		for (uint32_t d = 1u; d < 64u; d <<= 1) {
			const uint32_t below = __shfl_up(sum, d);
			if (lane >= d) sum += below;
		}
		if (bits) {
			const uint32_t off = at + sum - bits;
			const uint64_t v = code << (off & 31u);
			atomicOr(&sBits[off >> 5], (uint32_t)v);
			if (v >> 32) atomicOr(&sBits[(off >> 5) + 1u], (uint32_t)(v >> 32));
		}
		at += __shfl(sum, 63);
	}
	at += 7u;          /* end of block: seven zero bits */
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
	for (uint32_t d = 32u; d >= 1u; d >>= 1) { sumA += __shfl_xor(sumA, (int)d); sumB += __shfl_xor(sumB, (int)d); }
	if (lane == 0u) {
		uint32_t *const meta = segMeta + 4u * (size_t)blockIdx.x;
		meta[0] = bytes; meta[1] = sumA % CRX_ADLER; meta[2] = sumB % CRX_ADLER; meta[3] = 0u;
	}
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
