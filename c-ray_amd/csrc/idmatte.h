/*
 * idmatte.h — k_ids, k_ids_resolve, k_ids_matte: ID mattes — per pixel, which instances and which materials the camera rays hit first and how many of the pixel's samples
 * each one got (crh_render_ids, crh_ids_resolve, crh_ids_matte, include/cray_hip.h). The compositor's side of "what a denoiser or a compositor asks of a path tracer
 * besides the frame"; a capability beside the render path like aov.h: nothing of k_pathtrace_roll or k_aov includes or calls anything in here.
 *
 * Semantics. An ID buffer holds CRH_ID_WORDS = 16 words per pixel in the frame buffer's pixel order: id[0..5], count[0..5], lost, total, two reserved words no kernel in
 * here writes. For every pixel of the dispatch and every pass of it, in ascending pass order, the ray and the hit are k_aov's (aov.h: beginPath, then the walk of the
 * render kernels, a volume's free flight drawn from this path's sampler); the sample is the pair (instance id, material id) of the hit — DInstance::orig and
 * HitInfo::material, what crh_trace_rays reports as crh_hit.inst and crh_hit.material — or CRH_IDS_MISS twice. idFold below is the fold rule, word for word the header's:
 * nothing but integer compares, selects and adds, so every word of the buffer is predictable, and consecutive pass ranges compose bit for bit.
 *
 * Shape. k_aov's, and for its reason — the loop itself is k_aov's, firstHitWaves in aov.h; IdsKernel below is what k_ids brings to it: a wave pulls units of pixel groups from one counter; per chunk of up to 64 passes lane l walks pixel l / chunk, pass l % chunk and
 * leaves its two words in words 0 and 1 of its LDS column (AovStack: the walk's entries are dead by then); lane p then folds pixel p's samples in pass order. The chunks
 * of a pixel are folded by the same lane of the same wave one after the other, and a pixel belongs to one group of one unit: no atomics. The folding lane holds ONE
 * record — 14 words — in named registers (three 16-byte accesses and one of 8 bytes each way: the reserved words are neither read nor written). A group of up to 32
 * pixels (every dispatch of two passes or more) is folded by both halves of the wave at once, lane p the instance record of pixel p and lane 32 + p its material
 * record: the fold runs on as many lanes as the group has pixels — 4 of 64 at 16 passes —, so the second buffer costs wave time, not lanes (measured: DESIGN.md §3);
 * a larger group by lane p for both buffers in turn. Which buffers there are is a test of the kernel's arguments, not a template parameter. Nothing indexes the record
 * with a run-time value — the compare against all six ids gives six 0 / 1 words that are added to the six counts, the insertion compares `used` with every slot
 * index —, so the record never becomes scratch.
 *
 * ONE kernel, not k_aov's four instantiations: the walk is the rare-features one (volumes) for every scene, and the sampler is an argument (IdsRng below). The walk is
 * nine tenths of the kernel's 32 KB, four copies of it would have taken the library 70 KB past the 3 MiB tests/test_abi.py holds it under, and what the two
 * specialisations buy k_aov — registers for the albedo evaluator — k_ids does not need: 90 registers, no scratch, k_aov's LDS column (31 KB a workgroup): five waves
 * per SIMD.
 *
 * k_ids_resolve and k_ids_matte are one pixel per lane over the whole buffer, no scene: the ranking is a fixed 12-exchange sorting network on (count descending, slot
 * ascending) in registers; the matte's id list travels in the kernel's arguments (CRH_IDS_MATTE_MAX words: scalar loads).
 */
#pragma once

#define CRH_IDS_MISS 0xFFFFFFFFu
#ifndef CRH_IDS_WPS
#define CRH_IDS_WPS 5                                                /* waves per SIMD the register allocator leaves room for: what the LDS of k_aov's column admits */
#endif
static_assert(CRH_ID_SLOTS == 6 && CRH_ID_WORDS == 16, "IdRecord below is written for six slots in a 64-byte pixel");

struct alignas(16) IdQuad { uint32_t x, y, z, w; };
struct alignas(8) IdPair { uint32_t x, y; };

/* the 14 live words of a pixel, every one a named register */
struct IdRecord {
	uint32_t i0, i1, i2, i3, i4, i5;          /* id[0..5] */
	uint32_t c0, c1, c2, c3, c4, c5;          /* count[0..5] */
	uint32_t lost, total;
};
__device__ __forceinline__ IdRecord idLoad(const uint32_t *px) {
	const IdQuad a = ((const IdQuad *)px)[0], b = ((const IdQuad *)px)[1], c = ((const IdQuad *)px)[2];
	const IdPair d = ((const IdPair *)px)[6];
	return IdRecord{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y};
}
__device__ __forceinline__ void idStore(uint32_t *px, const IdRecord &r) {
	((IdQuad *)px)[0] = IdQuad{r.i0, r.i1, r.i2, r.i3};
	((IdQuad *)px)[1] = IdQuad{r.i4, r.i5, r.c0, r.c1};
	((IdQuad *)px)[2] = IdQuad{r.c2, r.c3, r.c4, r.c5};
	((IdPair *)px)[6] = IdPair{r.lost, r.total};
}
/* slots with a nonzero count (they are the front ones: slots fill front to back) */
__device__ __forceinline__ uint32_t idUsed(const IdRecord &r) {
	return (uint32_t)(r.c0 != 0u) + (uint32_t)(r.c1 != 0u) + (uint32_t)(r.c2 != 0u) + (uint32_t)(r.c3 != 0u) + (uint32_t)(r.c4 != 0u) + (uint32_t)(r.c5 != 0u);
}
/* One sample into the record (include/cray_hip.h, the fold rule). A miss: total alone. A hit with id s: the slot below `used` that holds s (the lowest one, should a
 * caller's record hold an id twice) gets the sample; no such slot: slot `used` becomes (s, 1) while one is free, `lost` counts the sample once none is. */
__device__ __forceinline__ void idFold(IdRecord &r, uint32_t &used, uint32_t s) {
	const uint32_t hit = (uint32_t)(s != CRH_IDS_MISS);
	const uint32_t m0 = (uint32_t)(used > 0u && r.i0 == s), m1 = (uint32_t)(used > 1u && r.i1 == s), m2 = (uint32_t)(used > 2u && r.i2 == s);
	const uint32_t m3 = (uint32_t)(used > 3u && r.i3 == s), m4 = (uint32_t)(used > 4u && r.i4 == s), m5 = (uint32_t)(used > 5u && r.i5 == s);
	const uint32_t b1 = m0, b2 = b1 | m1, b3 = b2 | m2, b4 = b3 | m3, b5 = b4 | m4, found = b5 | m5;          /* bj: a slot below j holds s */
	const uint32_t fresh = hit & (found ^ 1u);                  /* a hit no slot holds */
	const uint32_t ins = fresh & (uint32_t)(used < (uint32_t)CRH_ID_SLOTS);
	const uint32_t n0 = ins & (uint32_t)(used == 0u), n1 = ins & (uint32_t)(used == 1u), n2 = ins & (uint32_t)(used == 2u);
	const uint32_t n3 = ins & (uint32_t)(used == 3u), n4 = ins & (uint32_t)(used == 4u), n5 = ins & (uint32_t)(used == 5u);
	r.i0 = n0 ? s : r.i0; r.i1 = n1 ? s : r.i1; r.i2 = n2 ? s : r.i2; r.i3 = n3 ? s : r.i3; r.i4 = n4 ? s : r.i4; r.i5 = n5 ? s : r.i5;
	r.c0 += (hit & m0) + n0;
	r.c1 += (hit & m1 & (b1 ^ 1u)) + n1;
	r.c2 += (hit & m2 & (b2 ^ 1u)) + n2;
	r.c3 += (hit & m3 & (b3 ^ 1u)) + n3;
	r.c4 += (hit & m4 & (b4 ^ 1u)) + n4;
	r.c5 += (hit & m5 & (b5 ^ 1u)) + n5;
	r.lost += fresh & (ins ^ 1u);
	r.total += 1u;
	used += ins;
}

/* the pixel's `pc` samples of this chunk — word k of `col` and onwards, one word per lane column — into the pixel's record at px */
__device__ __forceinline__ void idFoldPixel(uint32_t *px, const lds_u32 *col, uint32_t pc) {
	IdRecord r = idLoad(px);
	uint32_t used = idUsed(r);
	for (uint32_t k = 0; k < pc; ++k) idFold(r, used, col[k]);
	idStore(px, r);
}

/* The sampler of a path whose kind — CRH_OPT_SAMPLER — is an argument of the kernel, not a template parameter of it: both kinds keep their state in 64 bits (pt_device.h:
 * RngT), and every draw is the named kind's, bit for bit. A wave-uniform branch per draw — the camera ray's few and a volume's free flights — buys one copy of the walk
 * for both samplers: the walk is nine tenths of k_ids' code, and tests/test_abi.py holds the library under 3 MiB. */
struct IdsRng { uint64_t state; uint32_t halton; };
__device__ __forceinline__ void initSampler(IdsRng &r, int pass, int maxPasses, uint32_t pixelIndex) {
	if (r.halton) { HaltonRng h; crh::initSampler(h, pass, maxPasses, pixelIndex); r.state = h.state; }
	else { Rng g; crh::initSampler(g, pass, maxPasses, pixelIndex); r.state = g.state; }
}
__device__ __forceinline__ float getDimension(IdsRng &r) {
	float v;
	if (r.halton) { HaltonRng h{r.state}; v = crh::getDimension(h); r.state = h.state; }
	else { Rng g{r.state}; v = crh::getDimension(g); r.state = g.state; }
	return v;
}

/* k_ids' sample: the two ids; of a miss, CRH_IDS_MISS twice */
struct IdsSample {
	uint32_t inst = CRH_IDS_MISS, mat = CRH_IDS_MISS;
	__device__ __forceinline__ void put(AovStack &stk) const { stk.put(0, inst); stk.put(1, mat); }
};
/* what k_ids brings to the wave loop (aov.h: firstHitWaves); either buffer may be null */
struct IdsKernel {
	typedef IdsRng Rng;
	typedef IdsSample Sample;
	static constexpr bool rare = true;
	uint32_t *idsInst, *idsMat;
	uint32_t halton;
	__device__ __forceinline__ void seed(IdsRng &r) const { r.halton = halton; }
	/* a group of up to 32 pixels (two passes or more) is folded by both halves of the wave at once — lane p the instance record of pixel p, lane 32 + p its material
	 * record —, a larger one by lane p for both buffers, one after the other */
	__device__ __forceinline__ uint32_t foldLane(uint32_t lane, uint32_t npix) const { return npix <= 32u ? (lane & 31u) : lane; }
	/* a surface, or a scattering event inside a volume: the instance's index in the scene description and the record's material */
	template <class LP, class Cnt>
	__device__ __forceinline__ void hit(const DScene &S, LP &lp, const Walk &w, AovStack &stk, Cnt &, IdsSample &s) const {
		s.inst = S.instances[w.hit.inst].orig;
		s.mat = finishHit<true, true>(S, lp.ro, lp.rd, w.hit, stk).material;
	}
	__device__ __forceinline__ void fold(size_t pixel, const lds_u32 *col, uint32_t pc, int, uint32_t lane, uint32_t npix) const {
		const bool halves = npix <= 32u;
		uint32_t b = halves ? lane >> 5 : 0u;                 /* 0: the instance buffer and word 0 of the columns, 1: the material buffer and word 1 */
		for (const uint32_t bEnd = halves ? b + 1u : 2u; b < bEnd; ++b) {          /* (one record live at a time) */
			uint32_t *const buf = b ? idsMat : idsInst;
			if (buf) idFoldPixel(buf + pixel * (size_t)CRH_ID_WORDS, col + b * CRH_BLOCK, pc);
		}
	}
};

/* halton: the sampler (CRH_SAMPLER_HALTON). idsInst / idsMat: the two buffers, either may be null (crh_render_ids). The walk is the rare-features one (volumes) for
 * every scene. */
__global__ __launch_bounds__(CRH_BLOCK, CRH_IDS_WPS) void k_ids(const DScene Sarg, const crh_render_params P, const AovUnits U, uint32_t *idsInstArg, uint32_t *idsMatArg,
                                                                 uint32_t halton, uint32_t rayFlags, uint32_t *ovfAll) {
	__shared__ uint32_t s_lane[CRH_AOV_LANE_WORDS * CRH_BLOCK];
	__shared__ __attribute__((aligned(16))) uint32_t s_inst0[CRH_AOV_INST_LDS ? CRH_INST_LDS0_MAX * 16u : 4u];
	const DScene S = globalize(Sarg);
	AovStack stk = aovStack(S, s_lane, s_inst0, ovfAll);
	firstHitWaves(S, P, U, rayFlags, stk, IdsKernel{(uint32_t *)(__attribute__((address_space(1))) uint32_t *)idsInstArg, (uint32_t *)(__attribute__((address_space(1))) uint32_t *)idsMatArg, halton});
}

/* ---- the consumers: one pixel per lane, no scene --------------------------------------------------------------------------------------------------------------- */
/* slot a ranks before slot b: the larger count; equal counts: the lower slot (the key is unique, so any sorting network gives the one order) */
__device__ __forceinline__ void idRankExchange(uint32_t &ca, uint32_t &sa, uint32_t &ia, uint32_t &cb, uint32_t &sb, uint32_t &ib) {
	const bool swap = cb > ca || (cb == ca && sb < sa);
	const uint32_t c = ca, s = sa, i = ia;
	ca = swap ? cb : ca; sa = swap ? sb : sa; ia = swap ? ib : ia;
	cb = swap ? c : cb; sb = swap ? s : sb; ib = swap ? i : ib;
}
__device__ __forceinline__ void idRankPair(float &id, float &coverage, uint32_t i, uint32_t c, float total, bool any) {
	const bool full = any && c != 0u;
	id = full ? (float)i : -1.0f;
	coverage = full ? (float)c / total : 0.0f;
}
/* out[pixel][rank] = ((float)id, (float)count / (float)total), an empty rank (-1, 0): crh_ids_resolve */
__global__ __launch_bounds__(CRH_BLOCK) void k_ids_resolve(const uint32_t *ids, f4 *out, uint64_t pixels) {
	const uint64_t p = (uint64_t)blockIdx.x * CRH_BLOCK + threadIdx.x;
	if (p >= pixels) return;
	IdRecord r = idLoad(ids + p * CRH_ID_WORDS);
	uint32_t s0 = 0u, s1 = 1u, s2 = 2u, s3 = 3u, s4 = 4u, s5 = 5u;
	/* the 12-exchange, 5-layer network for six keys */
	idRankExchange(r.c0, s0, r.i0, r.c5, s5, r.i5); idRankExchange(r.c1, s1, r.i1, r.c3, s3, r.i3); idRankExchange(r.c2, s2, r.i2, r.c4, s4, r.i4);
	idRankExchange(r.c1, s1, r.i1, r.c2, s2, r.i2); idRankExchange(r.c3, s3, r.i3, r.c4, s4, r.i4);
	idRankExchange(r.c0, s0, r.i0, r.c3, s3, r.i3); idRankExchange(r.c2, s2, r.i2, r.c5, s5, r.i5);
	idRankExchange(r.c0, s0, r.i0, r.c1, s1, r.i1); idRankExchange(r.c2, s2, r.i2, r.c3, s3, r.i3); idRankExchange(r.c4, s4, r.i4, r.c5, s5, r.i5);
	idRankExchange(r.c1, s1, r.i1, r.c2, s2, r.i2); idRankExchange(r.c3, s3, r.i3, r.c4, s4, r.i4);
	const bool any = r.total != 0u;
	const float total = (float)r.total;
	f4 a, b, c;
	idRankPair(a.x, a.y, r.i0, r.c0, total, any); idRankPair(a.z, a.w, r.i1, r.c1, total, any);
	idRankPair(b.x, b.y, r.i2, r.c2, total, any); idRankPair(b.z, b.w, r.i3, r.c3, total, any);
	idRankPair(c.x, c.y, r.i4, r.c4, total, any); idRankPair(c.z, c.w, r.i5, r.c5, total, any);
	out[3 * p] = a; out[3 * p + 1] = b; out[3 * p + 2] = c;
}

/* the list of crh_ids_matte, in the kernel's arguments */
struct IdsMatteList { uint32_t n; uint32_t ids[CRH_IDS_MATTE_MAX]; };
/* out[pixel] = (float)(samples of the non-empty slots whose id is in the list) / (float)total, 0 where total is 0: crh_ids_matte */
__global__ __launch_bounds__(CRH_BLOCK) void k_ids_matte(const uint32_t *ids, float *out, uint64_t pixels, const IdsMatteList L) {
	const uint64_t p = (uint64_t)blockIdx.x * CRH_BLOCK + threadIdx.x;
	if (p >= pixels) return;
	const IdRecord r = idLoad(ids + p * CRH_ID_WORDS);
	uint32_t m0 = 0u, m1 = 0u, m2 = 0u, m3 = 0u, m4 = 0u, m5 = 0u;          /* slot j's id is in the list (a duplicate in the list sets the same word again) */
	for (uint32_t k = 0; k < L.n; ++k) {
		const uint32_t s = L.ids[k];
		m0 |= (uint32_t)(r.i0 == s); m1 |= (uint32_t)(r.i1 == s); m2 |= (uint32_t)(r.i2 == s);
		m3 |= (uint32_t)(r.i3 == s); m4 |= (uint32_t)(r.i4 == s); m5 |= (uint32_t)(r.i5 == s);
	}
	const uint32_t n = ((m0 ? r.c0 : 0u) + (m1 ? r.c1 : 0u) + (m2 ? r.c2 : 0u)) + ((m3 ? r.c3 : 0u) + (m4 ? r.c4 : 0u) + (m5 ? r.c5 : 0u));          /* (an empty slot adds its count: 0) */
	out[p] = r.total != 0u ? (float)n / (float)r.total : 0.0f;
}
