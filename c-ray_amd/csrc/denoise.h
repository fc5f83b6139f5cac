/*
 * denoise.h — k_denoise_prepare / k_denoise_iter: an edge-avoiding à-trous wavelet filter for the frame, guided by the first-hit buffers of aov.h
 * (crh_denoise, include/cray_hip.h). A capability beside the render path, like k_aov: nothing of k_pathtrace_roll includes or calls anything in here.
 *
 * Semantics (include/cray_hip.h states the arithmetic operation by operation; tests/test_denoise.py restates it in NumPy float32 and holds these kernels to it
 * bit for bit — only correctly rounded + - * / sqrt, comparisons and fabsf in a fixed order, no libm, no contraction). Prepare (both kinds' through dnAlbedo,
 * dnIrradiance and dnGuideRecord) turns a pixel of the frame and of the guides into two 16-byte records: C = {irradiance r g b (the colour divided by the
 * albedo; a miss counts as albedo 1), its luminance} and G = {unit normal x y z, depth / coverage}. Iteration i filters C with the 5 x 5 B3-spline taps at step
 * 2^i, every tap weighted by how well its normal, depth and luminance agree with the centre's; G never changes. The last iteration multiplies the albedo back
 * in and writes the frame.
 *
 * Shape. One thread per pixel, 32 x 8 pixels per workgroup. A tap is two 16-byte reads, and the iteration kernel comes in three forms that differ only in
 * where the taps are read (the arithmetic is one function, dnTap; its guide weights, dnGuideWeights, are the variance kernels' too):
 *   direct (LS = 0)       every tap from global memory: the two planes of a 1280 x 720 frame are 29 MB — they stay in the Infinity Cache, a workgroup's
 *                         neighbourhood in L2 / L1;
 *   dense tile (LS = s)   the workgroup stages its tile plus a halo of 2 s records in LDS (16-byte writes) and reads the taps s records apart
 *                         (ds_read_b128; s-way bank conflicts for s >= 2: neighbouring lanes are 16 s bytes apart). (32 + 4 s) x (8 + 4 s) x 32 B:
 *                         13.5 / 20 / 36 / 80 KB for s = 1 / 2 / 4 / 8, more than the LDS holds at s = 16;
 *   sub-lattice (LS = 1, stride s)   the pixels with equal (x mod s, y mod s) form an image in which the taps are ONE apart: the workgroup takes 32 x 8 pixels
 *                         of one such image, stages 36 x 12 records whatever the step — conflict-free LDS reads, 1.7 staged records per pixel instead of up
 *                         to 25 — and pays with global reads that are 16 s bytes apart (the workgroups of the other residues read the rest of the lines).
 * The dense tile at s = 1 and the sub-lattice at stride 1 are the same launch. Which form each step uses was measured (profiles/denoise_rate.log, 1280 x 720,
 * microseconds per step 1 / 2 / 4 / 8 / 16): direct 68 / 67 / 66 / 65 / 65, dense 72 / 72 / 71 / 84 / -, sub-lattice 73 / 74 / 77 / 83 / 93. The direct gather
 * wins everywhere and is what crh_denoise launches (dnDefaultForm in cray_hip.hip): a tap is five correctly rounded divisions — some 80 VALU instructions beside
 * two 16-byte reads that the caches serve — so the kernel is bound by arithmetic, and staging buys nothing to pay for its barrier; the sub-lattice's strided
 * global reads cost more the larger the step. The product library keeps the LS = 1 tile besides (the GPU tier of the tests runs it); the dense tiles of the
 * steps 2, 4, 8 are built only for the A/B (-DCRH_DENOISE_ALL_FORMS) and the emulation tier. No packed-float instructions, no MFMA, no scratch; 30-42 VGPRs.
 *
 * The variance-guided filter (crh_denoise_variance; k_denoise_prepare_v / k_denoise_variance / k_denoise_iter_v at the end of this file) stops at luminance edges
 * in units of the pixel's own standard deviation instead of a fixed relative difference. The variance comes from a second frame buffer, the mean of the first h
 * of the n passes: Var(frame) ~ h / (n - h) (L(half) - L(frame))^2, one degree of freedom a pixel, which a guide-weighted 5 x 5 mean (k_denoise_variance) makes
 * usable; every iteration carries it along (V' = sum w^2 V / (sum w)^2). Its record is C = {irradiance r g b, variance}: a tap stays at two 16-byte reads and the
 * luminance is recomputed from the record (the same function of the same bits). Direct gather only (a tap is bound by its five divisions, as above); the per-pixel sqrt is outside the loop.
 */
#pragma once

#define CRH_DN_TW 32          /* the workgroup's tile: 32 x 8 pixels — a wave is two rows of 32, 512 contiguous bytes of each plane per row */
#define CRH_DN_TH 8
static_assert(CRH_DN_TW * CRH_DN_TH == CRH_BLOCK, "one thread per pixel of the tile");
#define CRH_DN_MAX_ITERATIONS 8
#if defined(CRH_WITH_ALT_KERNELS) && !defined(CRH_DENOISE_ALL_FORMS)
#define CRH_DENOISE_ALL_FORMS          /* the dense tiles of the steps 2, 4, 8: measured, not shipped (the product library holds the forms crh_denoise picks) */
#endif
#ifdef CRH_DENOISE_ALL_FORMS
#define CRH_DN_DENSE_MAX_STEP 8
#else
#define CRH_DN_DENSE_MAX_STEP 1
#endif
#define CRH_DN_EPS_ALBEDO 0.00390625f          /* 2^-8 */
#define CRH_DN_EPS_DEPTH 1e-6f
#define CRH_DN_EPS_LUM 1e-4f

struct DnParams {
	int32_t W, H;
	int32_t step;              /* 2^i: the distance between taps, in pixels */
	int32_t stride;            /* the distance between the tile's pixels: 1, or `step` in the sub-lattice form */
	float sigmaNormal, sigmaDepth, sigmaColor;          /* sigmaColor: already scaled by 2^-i */
};

__device__ __forceinline__ float dnLum(float r, float g, float b) { return ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b); }
__device__ __forceinline__ float dnMax(float a, float b) { return a > b ? a : b; }

/* the albedo a colour is divided by and multiplied with again: a miss counts as 1 (the background's radiance is not demodulated), never below 2^-8 */
__device__ __forceinline__ void dnAlbedo(const f4 a0, const f4 a1, float &r, float &g, float &b) {
	const float miss = 1.0f - a1.w;
	r = dnMax(a0.x + miss, CRH_DN_EPS_ALBEDO); g = dnMax(a0.y + miss, CRH_DN_EPS_ALBEDO); b = dnMax(a0.z + miss, CRH_DN_EPS_ALBEDO);
}

__device__ __forceinline__ float dnGuard(float v) { return (v > 0.0f && v < __builtin_inff()) ? v : 0.0f; }          /* NaN, inf, negative -> 0 */

/* G of a pixel from its two AOV records (albedo r g b, normal x | normal y z, depth, coverage): the unit normal (zero where there is none), depth / coverage */
__device__ __forceinline__ f4 dnGuideRecord(const f4 a0, const f4 a1) {
	const float nx = a0.w, ny = a1.x, nz = a1.y;
	const float nn = (nx * nx + ny * ny) + nz * nz;
	f4 g = f4{0.0f, 0.0f, 0.0f, 0.0f};
	if (nn > 0.0f) { const float len = sqrtf(nn); g.x = nx / len; g.y = ny / len; g.z = nz / len; }
	if (a1.w > 0.0f) g.w = a1.z / a1.w;
	return g;
}
/* a frame's pixel (px: its three floats), guarded and divided by the pixel's albedo */
__device__ __forceinline__ void dnIrradiance(const float *px, float ar, float ag, float ab, float &ir, float &ig, float &ib) {
	ir = dnGuard(px[0]) / ar; ig = dnGuard(px[1]) / ag; ib = dnGuard(px[2]) / ab;
}

/* Prepare: the records of every pixel; with out != null (a denoise of no iterations) the frame at once: (c / a) * a */
__global__ __launch_bounds__(CRH_BLOCK) void k_denoise_prepare(const float *fb, const float *aovArg, f4 *C, f4 *G, float *out, uint64_t pixels) {
	const uint64_t i = (uint64_t)blockIdx.x * CRH_BLOCK + threadIdx.x;
	if (i >= pixels) return;
	const f4 a0 = ((const f4 *)aovArg)[2 * i], a1 = ((const f4 *)aovArg)[2 * i + 1];          /* albedo r g b, normal x | normal y z, depth, coverage */
	float ar, ag, ab, ir, ig, ib;
	dnAlbedo(a0, a1, ar, ag, ab);
	dnIrradiance(fb + 3 * i, ar, ag, ab, ir, ig, ib);
	if (out) { out[3 * i] = ir * ar; out[3 * i + 1] = ig * ag; out[3 * i + 2] = ib * ab; return; }
	const f4 g = dnGuideRecord(a0, a1);
	C[i] = f4{ir, ig, ib, dnLum(ir, ig, ib)};
	G[i] = g;
}

struct DnAcc { float r, g, b, w; };

/* how well q's normal (wn) and depth (wz) agree with p's */
__device__ __forceinline__ void dnGuideWeights(const f4 Gp, const f4 Gq, const DnParams &P, float &wn, float &wz) {
	const float dx = Gp.x - Gq.x, dy = Gp.y - Gq.y, dz = Gp.z - Gq.z;
	const float d2 = (dx * dx + dy * dy) + dz * dz;
	const float t = dnMax(1.0f - P.sigmaNormal * d2, 0.0f);
	const float t2 = t * t;
	wn = t2 * t2;
	const float r = (fabsf(Gp.w - Gq.w) / (dnMax(Gp.w, Gq.w) + CRH_DN_EPS_DEPTH)) / P.sigmaDepth;
	wz = 1.0f / (1.0f + r * r);
}

/* one tap: q's colour weighted by the B3 coefficient h and by how well q's normal, depth and luminance agree with p's */
__device__ __forceinline__ void dnTap(DnAcc &acc, const f4 Cp, const f4 Gp, const f4 Cq, const f4 Gq, float h, const DnParams &P) {
	float wn, wz;
	dnGuideWeights(Gp, Gq, P, wn, wz);
	const float e = (Cp.w - Cq.w) / (P.sigmaColor * ((Cp.w + Cq.w) + CRH_DN_EPS_LUM));
	const float wc = 1.0f / (1.0f + e * e);
	const float w = ((h * wn) * wz) * wc;
	acc.r = acc.r + w * Cq.x; acc.g = acc.g + w * Cq.y; acc.b = acc.b + w * Cq.z;
	acc.w = acc.w + w;
}

/* One iteration. LS = 0: the direct form; LS >= 1: the tile forms — the taps LS records apart in an LDS image of the tile plus a halo of 2 LS records, whose
 * records are P.stride pixels apart (LS * P.stride == P.step). out != null: the last iteration — the albedo multiplied back in, the frame written. */
template <int LS>
__global__ __launch_bounds__(CRH_BLOCK) void k_denoise_iter(const f4 *Cin, const f4 *G, f4 *Cout, const float *aovArg, float *out, const DnParams P) {
	constexpr int PW = CRH_DN_TW + 4 * LS, PH = CRH_DN_TH + 4 * LS;          /* the LDS image */
	__shared__ f4 s_C[LS ? PW * PH : 1];
	__shared__ f4 s_G[LS ? PW * PH : 1];
	const int tx = (int)threadIdx.x % CRH_DN_TW, ty = (int)threadIdx.x / CRH_DN_TW;
	const int stride = LS ? P.stride : 1;
	/* the workgroup's tile: pixels ox + i * stride, oy + j * stride; the blocks of the `stride` residues of one stretch of the image are neighbours in the grid */
	const int ox = ((int)blockIdx.x / stride) * (CRH_DN_TW * stride) + (int)blockIdx.x % stride;
	const int oy = ((int)blockIdx.y / stride) * (CRH_DN_TH * stride) + (int)blockIdx.y % stride;
	const int x = ox + tx * stride, y = oy + ty * stride;
	if (LS) {
		for (int i = (int)threadIdx.x; i < PW * PH; i += CRH_BLOCK) {
			const int gx = ox + (i % PW - 2 * LS) * stride, gy = oy + (i / PW - 2 * LS) * stride;
			if (gx >= 0 && gx < P.W && gy >= 0 && gy < P.H) {          /* (cells outside the image are never read: the taps test the same bounds) */
				const size_t q = (size_t)gy * (size_t)P.W + (size_t)gx;
				s_C[i] = Cin[q];
				s_G[i] = G[q];
			}
		}
		__syncthreads();
	}
	if (x >= P.W || y >= P.H) return;
	const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
	const int cell = (2 * LS + ty) * PW + 2 * LS + tx;
	const f4 Cp = LS ? s_C[cell] : Cin[p], Gp = LS ? s_G[cell] : G[p];
	DnAcc acc = DnAcc{0.0f, 0.0f, 0.0f, 0.0f};
	const float k[3] = {0.375f, 0.25f, 0.0625f};          /* the B3 spline, by |offset| */
#pragma unroll 1
	for (int dy = -2; dy <= 2; ++dy) {          /* (a row of taps at a time: unrolled 25 times, each form is 16 KB of code, five divisions a tap) */
		const int qy = y + dy * P.step;
		const float ky = dy == 0 ? k[0] : (dy == 1 || dy == -1) ? k[1] : k[2];
#pragma unroll
		for (int dx = -2; dx <= 2; ++dx) {
			const int qx = x + dx * P.step;
			if (qx < 0 || qx >= P.W || qy < 0 || qy >= P.H) continue;
			const float h = k[dx < 0 ? -dx : dx] * ky;
			if (LS) {
				const int c = cell + dy * LS * PW + dx * LS;
				dnTap(acc, Cp, Gp, s_C[c], s_G[c], h, P);
			} else {
				const size_t q = (size_t)qy * (size_t)P.W + (size_t)qx;
				dnTap(acc, Cp, Gp, Cin[q], G[q], h, P);
			}
		}
	}
	const float ir = acc.r / acc.w, ig = acc.g / acc.w, ib = acc.b / acc.w;          /* (the centre tap alone weighs 9/64) */
	if (out) {
		float ar, ag, ab;
		dnAlbedo(((const f4 *)aovArg)[2 * p], ((const f4 *)aovArg)[2 * p + 1], ar, ag, ab);
		out[3 * p] = ir * ar; out[3 * p + 1] = ig * ag; out[3 * p + 2] = ib * ab;
	} else Cout[p] = f4{ir, ig, ib, dnLum(ir, ig, ib)};
}

/* ---- the variance-guided filter (crh_denoise_variance) ---------------------------------------------------------------------------------------------
 * Prepare: the records C = {I_r, I_g, I_b, 0} and G as above, and the raw variance of every pixel in a plane of its own (the prefilter cannot run in place):
 * scale (L(half) - L(frame))^2, NaN and anything above 2^100 -> 2^100 (a zero weight times an infinite variance would be a NaN). out != null: as above. */
#define CRH_DN_VARIANCE_MAX 0x1p100f

__global__ __launch_bounds__(CRH_BLOCK) void k_denoise_prepare_v(const float *fb, const float *half, const float *aovArg, f4 *C, f4 *G, float *Vraw, float *out, float scale, uint64_t pixels) {
	const uint64_t i = (uint64_t)blockIdx.x * CRH_BLOCK + threadIdx.x;
	if (i >= pixels) return;
	const f4 a0 = ((const f4 *)aovArg)[2 * i], a1 = ((const f4 *)aovArg)[2 * i + 1];
	float ar, ag, ab, ir, ig, ib, hr, hg, hb;
	dnAlbedo(a0, a1, ar, ag, ab);
	dnIrradiance(fb + 3 * i, ar, ag, ab, ir, ig, ib);
	if (out) { out[3 * i] = ir * ar; out[3 * i + 1] = ig * ag; out[3 * i + 2] = ib * ab; return; }
	dnIrradiance(half + 3 * i, ar, ag, ab, hr, hg, hb);
	const float d = dnLum(hr, hg, hb) - dnLum(ir, ig, ib);
	const float v = scale * (d * d);
	const f4 g = dnGuideRecord(a0, a1);
	C[i] = f4{ir, ig, ib, 0.0f};
	G[i] = g;
	Vraw[i] = v < CRH_DN_VARIANCE_MAX ? v : CRH_DN_VARIANCE_MAX;
}

/* The variance prefilter: the guide-weighted mean of the raw variance over the 5 x 5 neighbours (no spline coefficient), into the records' fourth component.
 * The centre's weight is 1, so the sum of the weights is at least 1. */
__global__ __launch_bounds__(CRH_BLOCK) void k_denoise_variance(const float *Vraw, const f4 *G, f4 *C, const DnParams P) {
	const int x = (int)blockIdx.x * CRH_DN_TW + (int)threadIdx.x % CRH_DN_TW, y = (int)blockIdx.y * CRH_DN_TH + (int)threadIdx.x / CRH_DN_TW;
	if (x >= P.W || y >= P.H) return;
	const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
	const f4 Gp = G[p];
	float acc = 0.0f, ws = 0.0f;
#pragma unroll 1
	for (int dy = -2; dy <= 2; ++dy) {
		const int qy = y + dy;
#pragma unroll
		for (int dx = -2; dx <= 2; ++dx) {
			const int qx = x + dx;
			if (qx < 0 || qx >= P.W || qy < 0 || qy >= P.H) continue;
			const size_t q = (size_t)qy * (size_t)P.W + (size_t)qx;
			float wn, wz;
			dnGuideWeights(Gp, G[q], P, wn, wz);
			const float wg = wn * wz;
			acc = acc + wg * Vraw[q];
			ws = ws + wg;
		}
	}
	((float *)(C + p))[3] = acc / ws;
}

/* One iteration, the direct form. P.sigmaColor is in standard deviations and is NOT scaled by the step: the variance shrinks by itself. The colour weight's
 * denominator is per pixel (the sqrt is outside the loop) but a tap still divides by it — the result depends on the division, not on a reciprocal —, so a tap is
 * five divisions like dnTap's, with two additions and a product fewer, five VALU instructions more for the luminance and three for the variance. */
__global__ __launch_bounds__(CRH_BLOCK) void k_denoise_iter_v(const f4 *Cin, const f4 *G, f4 *Cout, const float *aovArg, float *out, const DnParams P) {
	const int x = (int)blockIdx.x * CRH_DN_TW + (int)threadIdx.x % CRH_DN_TW, y = (int)blockIdx.y * CRH_DN_TH + (int)threadIdx.x / CRH_DN_TW;
	if (x >= P.W || y >= P.H) return;
	const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
	const f4 Cp = Cin[p], Gp = G[p];
	const float Lp = dnLum(Cp.x, Cp.y, Cp.z);
	const float den = P.sigmaColor * sqrtf(Cp.w) + CRH_DN_EPS_LUM;
	DnAcc acc = DnAcc{0.0f, 0.0f, 0.0f, 0.0f};
	float va = 0.0f;
	const float k[3] = {0.375f, 0.25f, 0.0625f};
#pragma unroll 1
	for (int dy = -2; dy <= 2; ++dy) {
		const int qy = y + dy * P.step;
		const float ky = dy == 0 ? k[0] : (dy == 1 || dy == -1) ? k[1] : k[2];
#pragma unroll
		for (int dx = -2; dx <= 2; ++dx) {
			const int qx = x + dx * P.step;
			if (qx < 0 || qx >= P.W || qy < 0 || qy >= P.H) continue;
			const float h = k[dx < 0 ? -dx : dx] * ky;
			const size_t q = (size_t)qy * (size_t)P.W + (size_t)qx;
			const f4 Cq = Cin[q];
			float wn, wz;
			dnGuideWeights(Gp, G[q], P, wn, wz);
			const float e = (Lp - dnLum(Cq.x, Cq.y, Cq.z)) / den;
			const float wc = 1.0f / (1.0f + e * e);
			const float w = ((h * wn) * wz) * wc;
			acc.r = acc.r + w * Cq.x; acc.g = acc.g + w * Cq.y; acc.b = acc.b + w * Cq.z;
			acc.w = acc.w + w;
			va = va + (w * w) * Cq.w;
		}
	}
	const float ir = acc.r / acc.w, ig = acc.g / acc.w, ib = acc.b / acc.w;
	if (out) {
		float ar, ag, ab;
		dnAlbedo(((const f4 *)aovArg)[2 * p], ((const f4 *)aovArg)[2 * p + 1], ar, ag, ab);
		out[3 * p] = ir * ar; out[3 * p + 1] = ig * ag; out[3 * p + 2] = ib * ab;
	} else Cout[p] = f4{ir, ig, ib, va / (acc.w * acc.w)};
}
