/*
 * despeckle.h — the firefly filter crx_despeckle (include/cray_hip_exr.h, which states the rule operation by operation; this file restates none of the reasons).
 * Included by exr_zip.hip behind png_pack.h (pngLum, crh::em::fbits).
 *   k_despeckle_measure<RADIUS>    one lane a pixel, 32 x 8 tiles. The workgroup stages its tile plus a halo of 2 — 36 x 12 pixels — in LDS: wave w takes rows 3 w .. 3 w + 2,
 *                                  lane l < 36 column l, three unconditional 12-byte loads a lane (36 lanes cover a contiguous 432-byte span of a row), and keeps of
 *                                  every pixel its limit (factor * g) + floor (-1 outside the image) and, for the pixel's own lane, g (-1 if bad). After that nothing
 *                                  but LDS is read: every pixel's three floats come from memory once, not 25 times, and the limit is computed once a pixel, not once a
 *                                  tap. A lane decides by the monotone count — fewer than k neighbours whose limit reaches g(p) — in a compare and an add a tap, m comes
 *                                  from the pixel's distance to the image's edges, and only a clamped lane selects T, the k-th largest limit (the limit of the k-th
 *                                  largest g: the limit is monotone), by counting over the same LDS window. The halo is 2 for both radii (one staging code); the radius
 *                                  is a template parameter, the window unrolled.
 *                                  Stats: the workgroup's counts, max and min meet in LDS and go to the four global words by at most four atomics a workgroup;
 *                                  integer adds, and max / min on the bits of floats >= 0, whose order is the floats': the result does not depend on scheduling.
 *   k_despeckle_apply              one lane four pixels of the plane (one 16-byte load); a frame's pixel is touched only where its scale is not 1, so a frame with
 *                                  few fireflies costs the plane's 4 bytes a pixel, not the frame's 24.
 * Only __syncthreads and 32-bit atomicAdd / atomicMax / atomicMin: the file compiles unmodified on tests/emu/hipemu.
 */
#pragma once
#include "png_display.h"

#define CRX_DESPECKLE_MAX_FRAMES 8u
#define CRX_DESPECKLE_FACTOR_MAX 1048576.0f          /* 2^20 */
#define CRX_DESPECKLE_FLOOR_MAX 1048576.0f
#define DS_TILE_W 32u
#define DS_TILE_H 8u
#define DS_HALO 2u
#define DS_LDS_W (DS_TILE_W + 2u * DS_HALO)          /* 36 */
#define DS_LDS_H (DS_TILE_H + 2u * DS_HALO)          /* 12 */

struct DsParams { float factor, floor; uint32_t rank; };
struct alignas(16) DsQuad { float s[4]; };

__device__ __forceinline__ bool dsFinite(float v) { return (crh::em::fbits(v) & 0x7f800000u) != 0x7f800000u; }
/* "any of r, g, b is a NaN or infinite, or L is" is "L is": the three weights are finite and not zero, so a NaN component makes L a NaN and an infinite one makes it
 * infinite or — against an infinity of the other sign — a NaN; nothing finite brings either back */
__device__ __forceinline__ bool dsBad(float lum) { return !dsFinite(lum); }
/* the k-th largest of the neighbours' limits around LDS index c, with multiplicity, 1 <= k <= m: from the top, each round takes the largest value below the last
 * one and how often it stands there, until k values are passed — at most k rounds of one pass over the window. On the bits as signed integers: the limits are
 * floats >= 0 (+inf included), whose order is their bits', and the outside's -1 is negative there and never taken. */
template <int RADIUS> __device__ float dsKthLargest(const float *sF, uint32_t c, uint32_t k) {
	int bound = 0x7fffffff, best = 0;
	uint32_t left = k;
#pragma unroll 1
	for (uint32_t round = 0; round < k; ++round) {
		uint32_t count = 0u;
		best = -1;
#pragma unroll
		for (int dy = -RADIUS; dy <= RADIUS; ++dy)
#pragma unroll
			for (int dx = -RADIUS; dx <= RADIUS; ++dx) {
				if ((dx | dy) == 0) continue;
				const int b = (int)crh::em::fbits(sF[(int)c + dy * (int)DS_LDS_W + dx]);
				if (b >= bound) continue;
				count = b > best ? 1u : count + (b == best ? 1u : 0u);
				best = b > best ? b : best;
			}
		if (count >= left) break;
		left -= count;
		bound = best;
	}
	return crh::em::ffrom((uint32_t)best);
}

/* plane: the scale s of every pixel [H, W]. stats: {clamped, bad, the bits of max_clamped, the bits of min_scale}, set to {0, 0, 0, the bits of 1} by the caller.
 * The grid is tilesX * ceil(H / 8) workgroups in one dimension. */
template <int RADIUS>
__global__ __launch_bounds__(256) void k_despeckle_measure(const float *guide, uint32_t width, uint32_t height, uint32_t tilesX, DsParams P, float *plane, uint32_t *stats) {
	__shared__ float sF[DS_LDS_H * DS_LDS_W];          /* (factor * g(q)) + floor of the tile and its halo; -1 outside the image */
	__shared__ float sG[DS_LDS_H * DS_LDS_W];          /* g(q); -1 for a bad pixel (read by the pixel's own lane only) */
	__shared__ uint32_t sStat[4];
	const uint32_t tid = threadIdx.x, by = blockIdx.x / tilesX, bx = blockIdx.x - by * tilesX;
	const int x0 = (int)(bx * DS_TILE_W) - (int)DS_HALO, y0 = (int)(by * DS_TILE_H) - (int)DS_HALO;
	if (tid < 4u) sStat[tid] = tid == 3u ? 0x3f800000u : 0u;
	{          /* staging: wave w takes rows 3 w .. 3 w + 2 of the 12, lane l < 36 column l; the three loads of a lane are unconditional (a lane outside reads pixel 0) */
		const uint32_t col = tid & 63u, row0 = (tid >> 6) * 3u;
		const int x = x0 + (int)col;
		const bool colIn = col < DS_LDS_W && x >= 0 && x < (int)width;
		float px[3][3];
		bool in[3];
#pragma unroll
		for (uint32_t k = 0; k < 3u; ++k) {
			const int y = y0 + (int)(row0 + k);
			in[k] = colIn && y >= 0 && y < (int)height;
			const float *const q = guide + 3u * (in[k] ? (size_t)y * width + (size_t)x : (size_t)0);
			px[k][0] = q[0]; px[k][1] = q[1]; px[k][2] = q[2];
		}
		if (col < DS_LDS_W) {
#pragma unroll
			for (uint32_t k = 0; k < 3u; ++k) {
				const float lum = pngLum(px[k][0], px[k][1], px[k][2]);
				const bool bad = dsBad(lum);
				const float g = !bad && lum > 0.0f ? lum : 0.0f;
				const uint32_t i = (row0 + k) * DS_LDS_W + col;
				sF[i] = in[k] ? (P.factor * g) + P.floor : -1.0f;
				sG[i] = bad ? -1.0f : g;
			}
		}
	}
	__syncthreads();
	const uint32_t tx = tid & (DS_TILE_W - 1u), ty = tid / DS_TILE_W, x = bx * DS_TILE_W + tx, y = by * DS_TILE_H + ty;
	if (x < width && y < height) {
		const uint32_t c = (ty + DS_HALO) * DS_LDS_W + tx + DS_HALO;
		const float own = sG[c];
		const bool bad = own < 0.0f;
		const float gp = bad ? 0.0f : own;
		uint32_t reach = 0u;          /* the neighbours whose limit reaches g(p); one outside the image (-1) never does */
#pragma unroll
		for (int dy = -RADIUS; dy <= RADIUS; ++dy)
#pragma unroll
			for (int dx = -RADIUS; dx <= RADIUS; ++dx) {
				if ((dx | dy) == 0) continue;
				reach += sF[(int)c + dy * (int)DS_LDS_W + dx] >= gp ? 1u : 0u;
			}
		/* m, the neighbours inside the image: the window cut at the image's edges, less the pixel itself */
		const uint32_t left = zipMin(x, (uint32_t)RADIUS), right = zipMin(width - 1u - x, (uint32_t)RADIUS), up = zipMin(y, (uint32_t)RADIUS), down = zipMin(height - 1u - y, (uint32_t)RADIUS);
		const uint32_t m = (left + right + 1u) * (up + down + 1u) - 1u, k = zipMin(P.rank, m);
		const bool clamped = !bad && reach < k;          /* (m == 0: k == 0, never) */
		float s = bad ? 0.0f : 1.0f;
		if (clamped) {
			s = dsKthLargest<RADIUS>(sF, c, k) / gp;          /* T: the k-th largest limit is the limit of the k-th largest g — the limit is monotone */
			atomicAdd(&sStat[0], 1u);
			atomicMax(&sStat[2], crh::em::fbits(gp));
			atomicMin(&sStat[3], crh::em::fbits(s));
		}
		if (bad) atomicAdd(&sStat[1], 1u);
		plane[(size_t)y * width + x] = s;
	}
	__syncthreads();
	if (tid == 0u) {
		if (sStat[0]) { atomicAdd(&stats[0], sStat[0]); atomicMax(&stats[2], sStat[2]); atomicMin(&stats[3], sStat[3]); }
		if (sStat[1]) atomicAdd(&stats[1], sStat[1]);
	}
}

/* pixel p of a frame under its scale: untouched where s == 1, three +0.0f where s == 0, c * s otherwise */
__device__ __forceinline__ void dsScalePixel(float *frame, size_t p, float s) {
	if (s == 1.0f) return;
	float *const c = frame + 3u * p;
	if (s == 0.0f) { c[0] = 0.0f; c[1] = 0.0f; c[2] = 0.0f; return; }
	c[0] = c[0] * s; c[1] = c[1] * s; c[2] = c[2] * s;
}

/* plane: `pixels` scales in a buffer of a multiple of four floats, 16-byte aligned (the context's own) */
__global__ __launch_bounds__(256) void k_despeckle_apply(const float *plane, uint32_t pixels, float *frame) {
	const uint32_t p = 4u * (blockIdx.x * 256u + threadIdx.x);          /* (pixels < 2^30) */
	if (p >= pixels) return;
	if (p + 4u <= pixels) {
		const DsQuad v = *(const DsQuad *)(plane + p);
		dsScalePixel(frame, p, v.s[0]); dsScalePixel(frame, p + 1u, v.s[1]); dsScalePixel(frame, p + 2u, v.s[2]); dsScalePixel(frame, p + 3u, v.s[3]);
	} else
		for (uint32_t q = p; q < pixels; ++q) dsScalePixel(frame, q, plane[q]);
}
