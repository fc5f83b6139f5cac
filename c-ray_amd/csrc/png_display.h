/*
 * png_display.h — the display transform of crx_png_pack_display and the automatic exposure crx_auto_exposure (include/cray_hip_exr.h, which states every operation
 * and constant; this file restates none of the reasons). Included by png_pack.h behind srgb8.h and exr_zip.h's helpers.
 *   k_png_convert_display<CURVE>   k_png_convert's shape — a lane makes one word of four consecutive image bytes — with exposure, the curve and the ordered dither
 *                                  between the float and srgb8.h's linearToSRGB. A word spans two pixels: the lane takes the component, column and row of its first
 *                                  byte from one division by 3 and one by W and steps them. The curve is a template parameter (a wave never sees two), the dither a
 *                                  wave-uniform flag. At most three divisions a component (Hable: h(2x)'s and the one by h(2 white); Reinhard: two), no LDS.
 *   k_png_histogram                a grid-stride pass over the pixels, four 12-byte loads in flight a lane; the luminance's bin (bits >> 19: sixteen bins an octave)
 *                                  is counted by atomicAdd in the workgroup's own 16 KB LDS histogram, whose non-zero bins go to the global one by return-less
 *                                  atomics. Integer counts: the result does not depend on scheduling.
 *   k_png_pick                     one workgroup of 256: the inclusive scan over the 4 096 bins, 256 at a time, in k_png_scan's pattern (within each wave, the
 *                                  waves' totals through LDS, the tiles before as a carry); the key bin is the number of bins whose cumulative count is below the
 *                                  rank — the counts are monotone —, counted by all lanes. No loop over the bins runs on one lane.
 * Only __shfl_up, __shfl_xor, __syncthreads and 32-bit atomicAdd: the file compiles unmodified on tests/emu/hipemu.
 */
#pragma once
#include "srgb8.h"

#define CRX_DISPLAY_X_MAX 1048576.0f          /* 2^20: past it every curve's byte is 255 */
#define CRX_EXPOSURE_MIN 0x1p-40f
#define CRX_EXPOSURE_MAX 0x1p40f
#define CRX_WHITE_MIN 0x1p-10f
#define CRX_WHITE_MAX 0x1p10f
#define CRX_HIST_BINS 4096u

/* what the convert kernel takes by value: white * white and h(2 * white) are computed once on the host, by pngHable below, so with the device's bits */
struct PngDisplay { float exposure, white2, hWhite; int dither; };

__host__ __device__ __forceinline__ float pngHable(float v) {
	return (v * (0.15f * v + 0.05f) + 0.004f) / (v * (0.15f * v + 0.5f) + 0.06f) - 0.02f / 0.3f;
}

/* y of x = exposure * c */
template <int CURVE> __device__ __forceinline__ float pngCurve(float x, const PngDisplay &d) {
	if (CURVE == CRX_CURVE_CLAMP) return x;
	x = x < CRX_DISPLAY_X_MAX ? x : CRX_DISPLAY_X_MAX;
	if (CURVE == CRX_CURVE_REINHARD) return (x * (1.0f + x / d.white2)) / (1.0f + x);
	if (CURVE == CRX_CURVE_ACES) return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
	return pngHable(2.0f * x) / d.hWhite;
}

/* the 8 x 8 Bayer index: for i = 0, 1, 2 bit 2 (2 - i) + 1 is bit i of x ^ y, bit 2 (2 - i) is bit i of y */
__host__ __device__ __forceinline__ uint32_t pngBayer(uint32_t x, uint32_t y) {
	const uint32_t q = x ^ y;
	uint32_t b = 0u;
	for (uint32_t i = 0; i < 3u; ++i) b |= ((q >> i) & 1u) << (2u * (2u - i) + 1u) | ((y >> i) & 1u) << (2u * (2u - i));
	return b;
}

/* t = linearToSRGB(y) * 255 to the byte: srgb8.h's truncation, or with the centred ordered offset in front of it */
__device__ __forceinline__ uint32_t pngDisplayByte(float t, int dither, uint32_t col, uint32_t row) {
	if (!dither) return (unsigned char)(t < 255.0f ? t : 255.0f);
	const float u = t + ((float)pngBayer(col & 7u, row & 7u) - 31.5f) / 64.0f;
	return u < 0.0f ? 0u : u < 255.0f ? (uint32_t)(unsigned char)u : 255u;
}

/* word wi of the 8-bit image [H, W, 3] under the display transform: bytes 4 wi .. 4 wi + 3 of `count` = 3 W H */
template <int CURVE>
__global__ __launch_bounds__(256) void k_png_convert_display(const float *fb, uint32_t count, uint32_t width, PngDisplay d, uint32_t *img) {
	const uint32_t wi = blockIdx.x * 256u + threadIdx.x;
	if (4u * (uint64_t)wi >= count) return;
	const uint32_t pixel = 4u * wi / 3u;
	uint32_t comp = 4u * wi - 3u * pixel, row = pixel / width, col = pixel - row * width, out = 0u;
	for (uint32_t b = 0; b < 4u && 4u * wi + b < count; ++b) {
		const float y = pngCurve<CURVE>(d.exposure * fb[4u * (size_t)wi + b], d);
		out |= pngDisplayByte(crh::linearToSRGB(y) * 255.0f, d.dither, col, row) << (8u * b);
		if (++comp == 3u) {
			comp = 0u;
			if (++col == width) { col = 0u; ++row; }
		}
	}
	img[wi] = out;
}

/* ---- automatic exposure ---- */
/* denoise.h's dnLum, restated: the two libraries share no code but srgb8.h and exact_math.h */
__device__ __forceinline__ float pngLum(float r, float g, float b) { return ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b); }

/* a pixel counts iff its luminance is finite and > 0 (a NaN fails the comparison), in bin bits >> 19 <= 4079 */
__device__ __forceinline__ void pngCount(uint32_t *sHist, float lum) {
	const uint32_t bits = crh::em::fbits(lum);
	if (lum > 0.0f && bits < 0x7f800000u) atomicAdd(&sHist[bits >> 19], 1u);
}

/* hist: CRX_HIST_BINS words, cleared by the caller. */
__global__ __launch_bounds__(256) void k_png_histogram(const float *fb, uint32_t pixels, uint32_t *hist) {
	__shared__ uint32_t sHist[CRX_HIST_BINS];
	for (uint32_t i = threadIdx.x; i < CRX_HIST_BINS; i += 256u) sHist[i] = 0u;
	__syncthreads();
	const uint32_t stride = gridDim.x * 256u;
	uint32_t p = blockIdx.x * 256u + threadIdx.x;
	for (; p + 3u * stride < pixels; p += 4u * stride) {          /* (pixels < 2^30, stride <= 2^18: no wrap) */          /* four pixels a lane, their loads unconditional: all in flight before the first is used */
		float lum[4];
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) {
			const float *const q = fb + 3u * (size_t)(p + k * stride);
			lum[k] = pngLum(q[0], q[1], q[2]);
		}
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) pngCount(sHist, lum[k]);
	}
	for (; p < pixels; p += stride) {          /* the rest: at most three a lane */
		const float *const q = fb + 3u * (size_t)p;
		pngCount(sHist, pngLum(q[0], q[1], q[2]));
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < CRX_HIST_BINS; i += 256u) {
		const uint32_t v = sHist[i];
		if (v) atomicAdd(&hist[i], v);
	}
}

/* One workgroup of 256. result: {the exposure's bits, the key's bits, the counted pixels, 0}. */
__global__ __launch_bounds__(256) void k_png_pick(const uint32_t *hist, uint32_t permille, float target, uint32_t *result) {
	__shared__ uint32_t sCum[CRX_HIST_BINS];
	__shared__ uint32_t sWave[4];
	__shared__ uint32_t sBelow;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if (threadIdx.x == 0u) sBelow = 0u;
	uint32_t carry = 0u;
	for (uint32_t base = 0u; base < CRX_HIST_BINS; base += 256u) {
		uint32_t e = hist[base + threadIdx.x];
		for (uint32_t d = 1u; d < 64u; d <<= 1) {
			const uint32_t o = __shfl_up(e, d);
			if (lane >= d) e += o;
		}
		if (lane == 63u) sWave[wave] = e;
		__syncthreads();
		uint32_t before = carry;
		for (uint32_t w = 0u; w < 4u; ++w) {
			if (w == wave) e += before;
			before += sWave[w];
		}
		sCum[base + threadIdx.x] = e;
		carry = before;
		__syncthreads();
	}
	const uint32_t counted = carry, rank = (uint32_t)(((uint64_t)counted * permille + 999u) / 1000u);          /* 1 .. counted where a pixel counts */
	uint32_t below = 0u;
	for (uint32_t i = threadIdx.x; i < CRX_HIST_BINS; i += 256u) below += sCum[i] < rank ? 1u : 0u;
	below = zipWaveSum(below);
	if (lane == 0u) atomicAdd(&sBelow, below);
	__syncthreads();
	if (threadIdx.x != 0u) return;
	float exposure = 1.0f, key = 0.0f;
	if (counted) {
		key = crh::em::ffrom(sBelow << 19 | 1u << 18);          /* the bin's midpoint */
		exposure = target / key;
		exposure = exposure < CRX_EXPOSURE_MIN ? CRX_EXPOSURE_MIN : exposure > CRX_EXPOSURE_MAX ? CRX_EXPOSURE_MAX : exposure;
	}
	result[0] = crh::em::fbits(exposure); result[1] = crh::em::fbits(key); result[2] = counted; result[3] = 0u;
}
