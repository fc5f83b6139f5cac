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
 * No packed-float instructions, no MFMA, no scratch; 1 KB of LDS. The enumeration, a thread's error sum and the copy are written once for both kernels of this file
 * (AdWalk, adErrorSum, adCopy), parameterised by the number of threads that share a rectangle.
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

/* The enumeration both kernels walk: the pixels t, t + STRIDE, ... of a rectangle `w` pixels wide (stored rows top to bottom, x ascending) for thread t of the STRIDE
 * that share the rectangle — the workgroup's CRH_BLOCK threads for a tile of k_adaptive_step, a wave's 64 lanes for a cell of k_adaptive_cells. The index advances
 * without a division (STRIDE = q w + r once). */
template <uint32_t STRIDE> struct AdWalk {
	uint32_t w, q, r, row, x;
	__device__ __forceinline__ AdWalk(uint32_t width, uint32_t t) : w(width), q(STRIDE / width), r(STRIDE % width), row(t / width), x(t % width) {}
	/* the first word of the pixel the walk stands on */
	__device__ __forceinline__ size_t word(size_t origin, size_t pitch) const { return origin + (size_t)row * pitch + (size_t)x * 3u; }
	/* on to the thread's next pixel */
	__device__ __forceinline__ void step() {
		row += q; x += r;
		if (x >= w) { x -= w; ++row; }
	}
};

/* thread t's partial sum: the errors of its pixels of the rectangle's n, added in that order */
template <uint32_t STRIDE>
__device__ __forceinline__ float adErrorSum(const float *fb, const float *half, size_t origin, size_t pitch, uint32_t w, uint32_t n, uint32_t t) {
	AdWalk<STRIDE> walk(w, t);
	float p = 0.0f;
#pragma unroll 4
	for (uint32_t k = t; k < n; k += STRIDE, walk.step()) p = p + adPixelError(fb, half, walk.word(origin, pitch));
	return p;
}

/* half := fb over the rectangle, raw bits, all three channels: a pixel a thread in the enumeration, four pixels' loads in flight before their stores (the compiler
 * may not move a load across a store to the other buffer itself). A pixel past the end reads the batch's first one again and stores nothing. */
template <uint32_t STRIDE>
__device__ __forceinline__ void adCopy(const uint32_t *src, uint32_t *dst, size_t origin, size_t pitch, uint32_t w, uint32_t n, uint32_t t) {
	AdWalk<STRIDE> walk(w, t);
#define CRH_AD_NEXT(at, ok, u) \
	const bool ok = k + (u) * STRIDE < n; \
	const size_t at = ok ? walk.word(origin, pitch) : at0; \
	walk.step();
#define CRH_AD_LOAD(v, at) const uint32_t v##r = src[at], v##g = src[at + 1], v##b = src[at + 2];
#define CRH_AD_STORE(v, at) { dst[at] = v##r; dst[at + 1] = v##g; dst[at + 2] = v##b; }
	for (uint32_t k = t; k < n; k += 4u * STRIDE) {
		const size_t at0 = walk.word(origin, pitch);          /* (k < n) */
		walk.step();
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

__global__ __launch_bounds__(CRH_BLOCK) void k_adaptive_step(const AdaptiveArgs A) {
	__shared__ float s_part[CRH_BLOCK];
	const uint32_t t = threadIdx.x;
	const crh_tile T = A.tiles[blockIdx.x];
	const uint32_t tw = (uint32_t)(T.x1 - T.x0), th = (uint32_t)(T.y1 - T.y0), n = tw * th;          /* (the host refuses empty tiles and tiles of more than 2^30 pixels) */
	const size_t origin = ((size_t)(A.H - T.y1) * (size_t)A.W + (size_t)T.x0) * 3u;                       /* the tile's first stored row, its first pixel */
	const size_t pitch = (size_t)A.W * 3u;
	bool cont = A.advanceAll != 0;
	if (!A.advanceAll) {
		const float p = adErrorSum<CRH_BLOCK>(A.fb, A.half, origin, pitch, tw, n, t);
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
	adCopy<CRH_BLOCK>((const uint32_t *)A.fb, (uint32_t *)A.half, origin, pitch, tw, n, t);
}

/* ---- k_adaptive_cells: the same step at cell granularity within each rectangle (crh_adaptive_step_cells, crh_render_adaptive_cells) ----------------------
 *
 * The rectangle stays the unit of work and of the interface; inside it the decision is made per cell of `cell` x `cell` pixels (anchored at the rectangle's first
 * stored row and first column; the last column and the last stored rows are ragged), optionally widened by one cell: a live cell goes on when it is hot — its
 * error is not <= the threshold — or, with `dilate`, when one of its up to eight neighbours in the same rectangle's grid is.
 *
 * One 256-thread workgroup per rectangle that holds a live cell; its four waves take the cells v, v + 4, ... . Lane l sums the errors of the cell's pixels
 * l, l + 64, ... in that order, and the 64 partials are folded by a __shfl_xor butterfly (strides 32 .. 1): float addition is commutative, so lane 0 — every
 * lane — ends with the bits of the tree the header states, and no barrier is needed inside a cell. E and the hot flag go to LDS (6 KB for 1024 cells), one
 * barrier; threads decide the cells t, t + 256, ... from the neighbours' flags and report; a second barrier; the waves copy their own cells that go on.
 * No packed-float instructions, no MFMA, no scratch.
 */
#define CRH_AD_CELLS_MAX 1024
#define CRH_AD_WAVE 64u
static_assert(CRH_AD_CELLS_MAX == CRH_ADAPTIVE_CELLS_MAX, "k_adaptive_cells: the LDS arrays hold one rectangle's cells");

struct AdaptiveCellsArgs {
	const float *fb;            /* [H, W, 3], never written */
	float *half;                /* [H, W, 3]: written over the cells that go on */
	const crh_tile *tiles;      /* one workgroup each: the rectangles that hold a live cell */
	const uint32_t *offsets;    /* per workgroup: the index of its rectangle's first cell in the three arrays below */
	const uint8_t *live;        /* per cell, or NULL: every cell is live */
	float *errors;              /* per cell */
	uint8_t *flags;             /* per cell: 1 = goes on */
	int W, H;
	int cell;
	float threshold;
	int dilate;
	int advanceAll;             /* crh_render_adaptive_cells' copies: no measurement, nothing reported, every live cell's half := fb */
};

__device__ __forceinline__ uint32_t adMin(uint32_t a, uint32_t b) { return a < b ? a : b; }

__global__ __launch_bounds__(CRH_BLOCK) void k_adaptive_cells(const AdaptiveCellsArgs A) {
	__shared__ float s_err[CRH_AD_CELLS_MAX];
	__shared__ uint8_t s_hot[CRH_AD_CELLS_MAX];          /* bit 0: hot, bit 1: live */
	__shared__ uint8_t s_go[CRH_AD_CELLS_MAX];
	const uint32_t t = threadIdx.x, wave = t / CRH_AD_WAVE, lane = t % CRH_AD_WAVE;
	const crh_tile T = A.tiles[blockIdx.x];
	const uint32_t first = A.offsets[blockIdx.x];
	const uint32_t tw = (uint32_t)(T.x1 - T.x0), th = (uint32_t)(T.y1 - T.y0), c = (uint32_t)A.cell;
	const uint32_t cx = (tw + c - 1u) / c, cy = (th + c - 1u) / c, cells = cx * cy;          /* (the host refuses rectangles of more than CRH_AD_CELLS_MAX cells) */
	const size_t origin = ((size_t)(A.H - T.y1) * (size_t)A.W + (size_t)T.x0) * 3u;          /* the rectangle's first stored row, its first pixel */
	const size_t pitch = (size_t)A.W * 3u;
	if (!A.advanceAll) {
		/* 1. the waves measure the cells wave, wave + 4, ... (everything but the lane's pixel is wave-uniform) */
		uint32_t i = wave % cx, j = wave / cx;
		for (uint32_t idx = wave; idx < cells; idx += CRH_BLOCK / CRH_AD_WAVE) {
			const bool isLive = !A.live || A.live[first + idx] != 0;
			float E = 0.0f;
			bool hot = false;
			if (isLive) {
				const uint32_t cw = adMin(c, tw - i * c), ch = adMin(c, th - j * c), n = cw * ch;
				const size_t at = origin + (size_t)(j * c) * pitch + (size_t)(i * c) * 3u;
				float p = adErrorSum<CRH_AD_WAVE>(A.fb, A.half, at, pitch, cw, n, lane);
#pragma unroll
				for (int stride = (int)CRH_AD_WAVE / 2; stride >= 1; stride >>= 1) p = p + __shfl_xor(p, stride);
				E = p / (float)n;
				hot = !(E <= A.threshold);
			}
			if (lane == 0) { s_err[idx] = E; s_hot[idx] = (uint8_t)((hot ? 1u : 0u) | (isLive ? 2u : 0u)); }
			i += CRH_BLOCK / CRH_AD_WAVE;
			while (i >= cx) { i -= cx; ++j; }
		}
		__syncthreads();
		/* 2. the threads decide the cells t, t + 256, ... from the neighbours' flags, and report */
		for (uint32_t idx = t; idx < cells; idx += CRH_BLOCK) {
			const uint32_t ci = idx % cx, cj = idx / cx;
			const uint32_t own = s_hot[idx];
			bool go = (own & 1u) != 0;
			if (A.dilate && (own & 2u) && !go) {
				const uint32_t i0 = ci ? ci - 1u : 0u, i1 = adMin(ci + 1u, cx - 1u), j0 = cj ? cj - 1u : 0u, j1 = adMin(cj + 1u, cy - 1u);
				for (uint32_t b = j0; b <= j1; ++b)
					for (uint32_t a = i0; a <= i1; ++a) go = go || (s_hot[b * cx + a] & 1u);
			}
			s_go[idx] = go ? 1 : 0;
			A.errors[first + idx] = s_err[idx];
			A.flags[first + idx] = go ? 1 : 0;
		}
		__syncthreads();
	}
	/* 3. the waves copy their own cells that go on */
	const uint32_t *src = (const uint32_t *)A.fb;
	uint32_t *dst = (uint32_t *)A.half;
	uint32_t i = wave % cx, j = wave / cx;
	for (uint32_t idx = wave; idx < cells; idx += CRH_BLOCK / CRH_AD_WAVE) {
		const bool go = A.advanceAll ? (!A.live || A.live[first + idx] != 0) : s_go[idx] != 0;
		if (go) {
			const uint32_t cw = adMin(c, tw - i * c), ch = adMin(c, th - j * c);
			adCopy<CRH_AD_WAVE>(src, dst, origin + (size_t)(j * c) * pitch + (size_t)(i * c) * 3u, pitch, cw, cw * ch, lane);
		}
		i += CRH_BLOCK / CRH_AD_WAVE;
		while (i >= cx) { i -= cx; ++j; }
	}
}
