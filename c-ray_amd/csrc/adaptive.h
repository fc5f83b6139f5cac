/* adaptive.h — k_adaptive_step: the per-tile error of a frame against its half-sample frame, the decision to go on, and the half-sample frame's advance
 * (crh_adaptive_step, crh_render_adaptive; include/cray_hip.h states the arithmetic operation by operation).
 *
 * Adaptive sampling at tile granularity sits beside the render path like k_aov and the denoise kernels: nothing in pathtrace_roll.h includes or calls it.
 * Consecutive pass ranges compose bit for bit and the result does not depend on the tile list, so a tile that stops at n passes holds exactly the uniform
 * n-pass render of its pixels. The error estimate costs no rays: `half` holds the mean of the first n / 2 of the frame's n passes, and
 * |frame - half| / sqrt(frame) averaged over the tile falls like the noise does. A tile that goes on renders passes [n, 2 n) next, so its new half-sample
 * frame is the frame it has now: the kernel copies it, tile by tile, right behind the reduction (the tile is fresh in L2).
 *
 * One 256-thread workgroup per tile. Thread t sums the errors of the pixels t, t + 256, ... of the tile's enumeration (stored rows top to bottom, x ascending)
 * in that order; the 256 partials are folded by a binary tree in LDS (strides 128 .. 1, a barrier per level: eight barriers a tile against 36 bytes of traffic a
 * pixel). The additions and their order are the interface; nothing else is. The pixel index advances without a division (256 = q tw + r once per workgroup).
 * No packed-float instructions, no MFMA, no scratch; 1 KB of LDS.
 */
#pragma once

#define CRH_AD_ERROR_MAX 0x1p100f
#define CRH_AD_EPS 1e-4f
static_assert(CRH_BLOCK == 256, "k_adaptive_step: the interface fixes 256 partial sums and the tree over them");

struct AdaptiveArgs {
	const float *fb;            /* [H, W, 3], never written */
	float *half;                /* [H, W, 3]: written over the tiles that go on */
	const crh_tile *tiles;      /* one workgroup each */
	float *errors;              /* per tile */
	uint32_t *flags;            /* per tile: 1 = goes on */
	int W, H;
	float threshold;
	int advanceAll;             /* crh_render_adaptive's first copy: no measurement, nothing reported, every tile's half := fb */
};

__device__ __forceinline__ float adPixelError(const float *fb, const float *half, size_t i) {
	const float fr = dnGuard(fb[i]), fg = dnGuard(fb[i + 1]), fbl = dnGuard(fb[i + 2]);
	const float ar = dnGuard(half[i]), ag = dnGuard(half[i + 1]), ab = dnGuard(half[i + 2]);
	const float d = (fabsf(fr - ar) + fabsf(fg - ag)) + fabsf(fbl - ab);
	const float s = (fr + fg) + fbl;
	const float e = d / sqrtf(s + CRH_AD_EPS);
	return e < CRH_AD_ERROR_MAX ? e : CRH_AD_ERROR_MAX;          /* NaN and overflow take the second branch */
}

__global__ __launch_bounds__(CRH_BLOCK) void k_adaptive_step(const AdaptiveArgs A) {
	__shared__ float s_part[CRH_BLOCK];
	const uint32_t t = threadIdx.x;
	const crh_tile T = A.tiles[blockIdx.x];
	const uint32_t tw = (uint32_t)(T.x1 - T.x0), th = (uint32_t)(T.y1 - T.y0), n = tw * th;          /* (the host refuses empty tiles and tiles of more than 2^30 pixels) */
	const size_t origin = ((size_t)(A.H - T.y1) * (size_t)A.W + (size_t)T.x0) * 3u;                       /* the tile's first stored row, its first pixel */
	const size_t pitch = (size_t)A.W * 3u;
	bool cont = A.advanceAll != 0;
	if (!A.advanceAll) {
		const uint32_t q = CRH_BLOCK / tw, r = CRH_BLOCK % tw;
		uint32_t row = t / tw, x = t % tw;
		float p = 0.0f;
#pragma unroll 4
		for (uint32_t k = t; k < n; k += CRH_BLOCK) {
			p = p + adPixelError(A.fb, A.half, origin + (size_t)row * pitch + (size_t)x * 3u);
			row += q; x += r;
			if (x >= tw) { x -= tw; ++row; }
		}
		s_part[t] = p;
		__syncthreads();
#pragma unroll
		for (uint32_t stride = CRH_BLOCK / 2; stride >= 1u; stride >>= 1) {
			if (t < stride) s_part[t] = s_part[t] + s_part[t + stride];
			__syncthreads();
		}
		const float E = s_part[0] / (float)n;
		cont = !(E <= A.threshold);
		if (t == 0) { A.errors[blockIdx.x] = E; A.flags[blockIdx.x] = cont ? 1u : 0u; }
	}
	if (!cont) return;
	/* half := fb over the tile, raw bits, all three channels: a pixel a thread in the enumeration above, four pixels' loads in flight before their stores (the
	 * compiler may not move a load across a store to the other buffer itself). A pixel past the end reads the batch's first one again and stores nothing. */
	const uint32_t *src = (const uint32_t *)A.fb;
	uint32_t *dst = (uint32_t *)A.half;
	const uint32_t q = CRH_BLOCK / tw, r = CRH_BLOCK % tw;
	uint32_t row = t / tw, x = t % tw;
#define CRH_AD_NEXT(at, ok, u) \
	const bool ok = k + (u) * CRH_BLOCK < n; \
	const size_t at = ok ? origin + (size_t)row * pitch + (size_t)x * 3u : at0; \
	row += q; x += r; \
	if (x >= tw) { x -= tw; ++row; }
#define CRH_AD_LOAD(v, at) const uint32_t v##r = src[at], v##g = src[at + 1], v##b = src[at + 2];
#define CRH_AD_STORE(v, at) { dst[at] = v##r; dst[at + 1] = v##g; dst[at + 2] = v##b; }
	for (uint32_t k = t; k < n; k += 4u * CRH_BLOCK) {
		CRH_AD_NEXT(at0, ok0, 0u)
		CRH_AD_NEXT(at1, ok1, 1u)
		CRH_AD_NEXT(at2, ok2, 2u)
		CRH_AD_NEXT(at3, ok3, 3u)
		CRH_AD_LOAD(v0, at0) CRH_AD_LOAD(v1, at1) CRH_AD_LOAD(v2, at2) CRH_AD_LOAD(v3, at3)
		CRH_AD_STORE(v0, at0)
		if (ok1) CRH_AD_STORE(v1, at1)
		if (ok2) CRH_AD_STORE(v2, at2)
		if (ok3) CRH_AD_STORE(v3, at3)
	}
#undef CRH_AD_NEXT
#undef CRH_AD_LOAD
#undef CRH_AD_STORE
}
