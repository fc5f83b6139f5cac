/*
 * aov.h — k_aov: the guide buffers a denoiser or a compositor asks of a path tracer — albedo, normal, depth and coverage of every camera ray's FIRST hit
 * (crh_render_aov, include/cray_hip.h). A capability beside the render path: nothing of k_pathtrace_roll includes or calls anything in here.
 *
 * Semantics. An AOV buffer holds CRH_AOV_CHANNELS = 8 floats per pixel in the frame buffer's pixel order (texture.c:24-28): albedo r g b, normal x y z, depth,
 * coverage. For every pixel of the dispatch and every pass of it, the ray is the one crh_render_region starts for that (x, y, pass) — beginPath: initSampler +
 * getCameraRay (renderer.c:280-284), the sampler the context's CRH_OPT_SAMPLER names — and the hit is getClosestIsect's over the reference's binary trees
 * (pathtrace.c:26-30), with the lane code of the render kernels: walkBegin / stepNodeAny / stepTri / stepCtrl, degenerate slabs as CRH_OPT_RENDER_SLABS says, a
 * volume's free flight drawn from this path's sampler where the render draws it. The sample of a miss is eight zeros; of a hit: coverage 1, depth = the record's
 * distance, normal = the record's surfaceNormal as finishHit leaves it (world space, not turned towards the viewer, a sphere's not renormalised: crh_hit.normal),
 * albedo as below; of a scattering event inside a volume: the same with normal (0, 0, 0), because the reference's is a placeholder (instance.c:81-88). Every
 * channel goes through the running mean of foldSample (renderer.c:288-291) in pass order, so consecutive pass ranges compose bit for bit.
 *
 * Albedo: a pure function of the hit — no sampler draws — on the material's bsdf graph. C = evalColor, V = evalValue at the hit:
 *   diffuse, metal, glass, transparent, isotropic   C(a)
 *   emission                                        C(a) * V(b)
 *   plastic                                         albedo of its diffuse layer c
 *   mix                                             cmix(albedo(a), albedo(b), V(c))
 *   add                                             albedo(a) + albedo(b)
 * evaluated iteratively: a mix / add node opens a frame, its a branch is evaluated, the result waits in the frame while the b branch is evaluated. At most
 * CRH_AOV_STACK frames are open at a time; the scene compiler reports the deepest nesting under a material's root (CompiledScene::max_albedo_depth), and a
 * scene that nests deeper makes crh_render_aov answer CRH_ERR_UNSUPPORTED.
 *
 * Shape (firstHitWaves below: k_aov and k_ids share the loop and differ in the sample and its fold). A wave takes `group` = 64 / min(passes, 64) consecutive pixels of a tile (row by row) at a time, for all passes of the dispatch; it pulls units of a few
 * such groups from an atomic counter (one group per pull was measured: 230 000 pulls of ONE counter bounded the 1280 x 720 x 16 dispatch at 2.76 ms whatever the
 * occupancy; the host sizes the units so that a wave gets about eight). Per chunk of up to 64 passes, lane l takes pixel l / chunk, pass l % chunk (pixel-major, like decodeItem: the passes of a pixel sit in neighbouring
 * lanes — coherent rays), walks its ray from start to end (one ray per lane, traverse()'s loop: walkToShade), and leaves its eight floats in LDS; lane p then folds pixel p's
 * samples in pass order into the buffer (two 16-byte loads, two 16-byte stores). The chunks of a pixel are folded by the same lane of the same wave one after
 * the other, so the order needs no atomics. A lane owns one 27-word column of LDS: 12 traversal-stack entries + the 15 park slots while it walks (deeper
 * entries: the wave's overflow columns in global memory, as in the render kernels), the albedo frames (8 node words, then 3 colour words per frame: six frames
 * in the column, the seventh and eighth in the overflow column) while it shades, its sample (8 words) while the wave folds. 31.5 KB of LDS per workgroup and
 * fewer than 96 registers: five waves per SIMD, against the four of a 32-word column (measured: profiles/aov_rate.log).
 */
#pragma once

#define CRH_AOV_STACK CRH_AOV_ALBEDO_DEPTH                            /* open mix / add frames of the albedo evaluator (cray_hip.h: 8) */
#ifndef CRH_AOV_LANE_WORDS
#define CRH_AOV_LANE_WORDS 27                                        /* a lane's LDS column: with the instance records and powf's tables 31.5 KB per workgroup, five workgroups per CU */
#endif
#ifndef CRH_AOV_WPS
#define CRH_AOV_WPS 5                                                /* waves per SIMD the register allocator leaves room for (the instantiations without rare features) */
#endif
#ifndef CRH_AOV_INST_LDS
#define CRH_AOV_INST_LDS 1                                           /* line 0 of the instance records staged in LDS (scenes of <= CRH_INST_LDS0_MAX instances) */
#endif
#ifndef CRH_AOV_BLOCKS_PER_CU
#define CRH_AOV_BLOCKS_PER_CU 5                                      /* workgroups the launch provides per CU */
#endif
#define CRH_AOV_STACK_LDS (CRH_AOV_LANE_WORDS - CRH_PARK_SLOTS)      /* traversal-stack entries in it (deeper ones: the wave's overflow columns) */
static_assert(CRH_AOV_STACK_LDS >= 6 && CRH_AOV_CHANNELS <= CRH_AOV_LANE_WORDS, "the walk's entries and the sample fit in the lane's column");
static_assert((CRH_AOV_STACK * 4 - CRH_AOV_LANE_WORDS) * 64 <= (int)CRH_OVF_WORDS_PER_WAVE, "the overflow columns hold the albedo frames the column does not");
static_assert((134 - CRH_AOV_STACK_LDS) * 64 <= (int)CRH_OVF_WORDS_PER_WAVE, "the overflow columns hold the deepest walk");

struct AovStack {
	lds_u32 *col;              /* &s_lane[threadIdx.x]: word i of this lane's column at col[i * CRH_BLOCK] (bank = lane mod 32) */
	glb_u32 *ovf;              /* wave-uniform: the wave's overflow columns */
	const lds_u32 *inst0;      /* workgroup-uniform: line 0 of the instance records (scenes of <= CRH_INST_LDS0_MAX instances), or null */
	const lds_u32 *waveCols;   /* the column of lane l of this wave: waveCols + l (what a folding lane reads) */
	__device__ __forceinline__ InstLine instLine(const DScene &S, int32_t idx, int line) const {
		if (line == 0 && inst0) {
			const lds_u32 *p = inst0 + (uint32_t)idx * 16u;
			return InstLine{ldsLoadF4(p), ldsLoadF4(p + 4), ldsLoadF4(p + 8), ldsLoadF4(p + 12)};
		}
		const f4 *g = (const f4 *)(S.instances + idx) + 4 * line;
		return InstLine{g[0], g[1], g[2], g[3]};
	}
	__device__ __forceinline__ void park(int i, uint32_t v) { col[(CRH_AOV_STACK_LDS + i) * CRH_BLOCK] = v; }
	__device__ __forceinline__ uint32_t unpark(int i) { return col[(CRH_AOV_STACK_LDS + i) * CRH_BLOCK]; }
	__device__ __forceinline__ void push(uint32_t i, uint32_t v) {
		if (__builtin_expect(i < (uint32_t)CRH_AOV_STACK_LDS, 1)) col[i * CRH_BLOCK] = v;
		else ovf[(i - (uint32_t)CRH_AOV_STACK_LDS) * 64u + (threadIdx.x & 63u)] = v;
	}
	__device__ __forceinline__ uint32_t pop(uint32_t i) {
		uint32_t v;
		if (__builtin_expect(i < (uint32_t)CRH_AOV_STACK_LDS, 1)) v = col[i * CRH_BLOCK];
		else v = ovf[(i - (uint32_t)CRH_AOV_STACK_LDS) * 64u + (threadIdx.x & 63u)];
		return v;
	}
	/* after the walk the column — and behind it the lane's overflow column — is free: word i of it (the albedo frames; the sample is words 0..7) */
	__device__ __forceinline__ void put(uint32_t i, uint32_t v) {
		if (__builtin_expect(i < (uint32_t)CRH_AOV_LANE_WORDS, 1)) col[i * CRH_BLOCK] = v;
		else ovf[(i - (uint32_t)CRH_AOV_LANE_WORDS) * 64u + (threadIdx.x & 63u)] = v;
	}
	__device__ __forceinline__ uint32_t get(uint32_t i) const {
		uint32_t v;
		if (__builtin_expect(i < (uint32_t)CRH_AOV_LANE_WORDS, 1)) v = col[i * CRH_BLOCK];
		else v = ovf[(i - (uint32_t)CRH_AOV_LANE_WORDS) * 64u + (threadIdx.x & 63u)];
		return v;
	}
};
/* a lane's stack over the workgroup's LDS arrays — CRH_AOV_LANE_WORDS * CRH_BLOCK words of columns, the instance records' line 0 (stageInstLine0: walk_machine.h) */
template <size_t NL, size_t NI>
__device__ __forceinline__ AovStack aovStack(const DScene &S, uint32_t (&s_lane)[NL], uint32_t (&s_inst0)[NI], uint32_t *ovfAll) {
	const uint32_t wave = (blockIdx.x * CRH_BLOCK + threadIdx.x) >> 6;
	AovStack stk;
	stk.col = (lds_u32 *)&s_lane[threadIdx.x];
	stk.ovf = (glb_u32 *)ovfAll + (size_t)__builtin_amdgcn_readfirstlane(wave) * CRH_OVF_WORDS_PER_WAVE;
	stk.inst0 = CRH_AOV_INST_LDS ? stageInstLine0(S, s_inst0) : nullptr;
	stk.waveCols = (const lds_u32 *)&s_lane[threadIdx.x & ~63u];
	return stk;
}
template <bool RARE> struct AovCounters { static constexpr int level = 0; static constexpr bool programs = RARE; static constexpr bool wide = false; };

/* The albedo of a hit (the header comment): frame f of the evaluator is word f of the lane's column (the mix / add node, bit 31 = its a branch is done) and
 * words 8 + 3 f .. of it (the a branch's colour). Depth <= CRH_AOV_STACK is the host's promise (crh_render_aov). Every turn of the loop evaluates at most one
 * colour operand and one value operand, each at ONE site: the image fetch and the program interpreter are inlined once per operand class, not once per node kind
 * (sampleBsdf does the same; three sites instead of two made the library 56 KB larger). */
template <class Cnt>
__device__ __forceinline__ void evalAlbedo(const DScene &S, uint32_t root, const ShadeRec &rec, Cnt &cnt, AovStack &stk, float &outR, float &outG, float &outB) {
	uint32_t sp = 0, cur = root;
	bool down = true;                     /* on the way down to a leaf; otherwise closing frames with the colour in hand */
	rgba col = rgba{0.0f, 0.0f, 0.0f, 0.0f};
	for (;;) {
		uint32_t vop = 0;                 /* the value operand this turn needs: an emission's strength (emission.c:46) or a mix's factor (mix.c:45) */
		bool needV = false, isMix = false;
		rgba A = rgba{0.0f, 0.0f, 0.0f, 0.0f};
		if (down) {
			const DBsdf n = loadBsdf(S, stk, cur);
			if (n.kind == CRH_BSDF_MIX || n.kind == CRH_BSDF_ADD) { stk.put(sp++, cur); cur = n.a; continue; }
			if (n.kind == CRH_BSDF_PLASTIC) { cur = n.c; continue; }          /* plastic.c:66-86: the diffuse layer below the coat */
			col = evalColor(S, n.a, rec, cnt, stk);
			if (n.kind == CRH_BSDF_EMISSION) { vop = n.b; needV = true; }
			down = false;
		} else {
			if (sp == 0) { outR = col.r; outG = col.g; outB = col.b; return; }
			const uint32_t top = stk.get(sp - 1u);
			if (!(top & 0x80000000u)) {      /* the a branch is done: its colour waits in the frame while the b branch is evaluated */
				stk.put(sp - 1u, top | 0x80000000u);
				stk.put(CRH_AOV_STACK + 3u * (sp - 1u), asU32(col.r)); stk.put(CRH_AOV_STACK + 3u * (sp - 1u) + 1u, asU32(col.g)); stk.put(CRH_AOV_STACK + 3u * (sp - 1u) + 2u, asU32(col.b));
				cur = loadBsdf(S, stk, top).b;
				down = true;
				continue;
			}
			--sp;
			const DBsdf m = loadBsdf(S, stk, top & 0x7FFFFFFFu);
			A = rgba{asF32(stk.get(CRH_AOV_STACK + 3u * sp)), asF32(stk.get(CRH_AOV_STACK + 3u * sp + 1u)), asF32(stk.get(CRH_AOV_STACK + 3u * sp + 2u)), 0.0f};
			if (m.kind == CRH_BSDF_MIX) { vop = m.c; needV = true; isMix = true; }
			else col = cadd(A, col);                                          /* add.c:42-49 */
		}
		if (needV) {
			const float v = evalValue(S, vop, rec, cnt, stk);
			col = isMix ? cmix(A, col, v) : ccoef(v, col);                    /* color.h:46 */
		}
	}
}

/* the work of a dispatch: the pixels of a tile list, tile by tile and row by row inside a tile, in units of `groups` x `group` consecutive pixels of one tile */
struct AovUnits {
	const crh_tile *tiles;
	const uint32_t *start;     /* start[t] = first unit of tile t; start[ntiles] = total */
	uint32_t ntiles, total;
	uint32_t *counter;
	uint32_t group;            /* pixels a wave takes at a time: 64 / min(pass_count, 64) */
	uint32_t groups;           /* such groups per unit (consecutive ones of a tile) */
};

/* The wave loop of a first-hit kernel (k_aov below; k_ids: idmatte.h) — the header's Shape, written once: the pull of a unit, its tile, the groups, the chunks of up to
 * 64 passes, the pixel-major lane assignment, the lane's walk, the two fence / lock-step pairs around the fold. What the kernels differ in comes with K:
 *   K::Rng, seed(rng)       the paths' sampler, and what it holds besides the state beginPath seeds (IdsRng's kind)
 *   K::rare                 node programs or volumes in the walk, as in k_pathtrace_roll
 *   K::Sample               what a lane leaves in its column: constructed as a miss, put(stk) writes it
 *   hit(S, lp, w, stk, cnt, s)   fills it from a finished walk that hit (w.hit.inst >= 0)
 *   foldLane(lane, npix)    which of the group's npix pixels this lane folds (>= npix: none)
 *   fold(pixel, col, pc, p0, lane, npix)   the folding lane: its pixel's index in the buffer, the column of the pixel's first sample of this chunk (sample k, word i:
 *                           col[i * CRH_BLOCK + k]), the chunk's passes p0 .. p0 + pc
 * stk: the lane's column over the workgroup's LDS (aovStack). */
template <class K>
__device__ __forceinline__ void firstHitWaves(const DScene &S, const crh_render_params &P, const AovUnits &U, uint32_t rayFlags, AovStack &stk, const K &kern) {
	const crh_tile *const tiles = asGlobal(U.tiles);
	const uint32_t *const start = asGlobal(U.start);
	const uint32_t lane = threadIdx.x & 63u;
	const lds_u32 *const waveCols = stk.waveCols;
	const int passEnd = P.first_pass + P.pass_count;
	for (;;) {
		uint32_t u = 0;
		if (lane == 0) u = atomicAdd((uint32_t *)(__attribute__((address_space(1))) uint32_t *)U.counter, 1u);
		u = __builtin_amdgcn_readfirstlane(u);
		if (u >= U.total) break;
		uint32_t lo = 0, hi = U.ntiles;          /* (wave-uniform) the tile of unit u */
		while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (start[mid] <= u) lo = mid; else hi = mid; }
		const crh_tile t = tiles[lo];
		const uint32_t tw = (uint32_t)(t.x1 - t.x0), tilePixels = tw * (uint32_t)(t.y1 - t.y0);
		for (uint32_t gi = 0; gi < U.groups; ++gi) {
		const uint32_t first = ((u - start[lo]) * U.groups + gi) * U.group;                     /* the group's first pixel, counted inside the tile */
		if (first >= tilePixels) break;
		const uint32_t npix = min(U.group, tilePixels - first);
		/* the pixel this lane FOLDS (fl < npix) */
		const uint32_t fl = kern.foldLane(lane, npix);
		const uint32_t fIdx = first + min(fl, npix - 1u);
		const int fx = t.x0 + (int)(fIdx % tw), fy = t.y0 + (int)(fIdx / tw);
		const size_t fPixel = (size_t)fx + (size_t)(P.image_height - (fy + 1)) * (size_t)P.image_width;
		for (int p0 = P.first_pass; p0 < passEnd; p0 += 64) {
			const uint32_t pc = (uint32_t)min(64, passEnd - p0);
			const uint32_t pj = lane / pc;                                                      /* pixel-major: the passes of a pixel in neighbouring lanes */
			typename K::Sample s;
			if (pj < npix) {
				const uint32_t idx = first + pj;
				const int x = t.x0 + (int)(idx % tw), y = t.y0 + (int)(idx / tw), pass = p0 + (int)(lane - pj * pc);
				AovCounters<K::rare> cnt;
				LanePathT<typename K::Rng> lp;
				memset(&lp, 0, sizeof(lp));
				kern.seed(lp.r.rng);
				beginPath(S, P, x, y, pass, lp.ro, lp.rd, lp.r, cnt);
				auto port = lanePort(lp);
				Walk w;
				walkBegin(S, w, stk, lp.ro, lp.rd, cnt, port, rayFlags);
				walkToShade(S, w, stk, cnt, port);
				if (w.hit.inst >= 0) kern.hit(S, lp, w, stk, cnt, s);
			}
			s.put(stk);
			__threadfence_block();                 /* the samples of all lanes are visible to the folding lanes */
			CRH_LOCKSTEP();
			if (fl < npix) kern.fold(fPixel, waveCols + fl * pc, pc, p0, lane, npix);
			__threadfence_block();                 /* ... and read before the next chunk's walks overwrite them */
			CRH_LOCKSTEP();
		}
		}
	}
}

/* k_aov's sample: the eight floats; of a miss, eight zeros */
struct AovSample {
	float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, s4 = 0.0f, s5 = 0.0f, s6 = 0.0f, s7 = 0.0f;
	__device__ __forceinline__ void put(AovStack &stk) const {
		stk.put(0, asU32(s0)); stk.put(1, asU32(s1)); stk.put(2, asU32(s2)); stk.put(3, asU32(s3));
		stk.put(4, asU32(s4)); stk.put(5, asU32(s5)); stk.put(6, asU32(s6)); stk.put(7, asU32(s7));
	}
};
template <int SAMP, bool RARE> struct AovKernel {
	typedef RngT<SAMP> Rng;
	typedef AovSample Sample;
	static constexpr bool rare = RARE;
	f4 *aov;
	__device__ __forceinline__ void seed(Rng &) const {}
	__device__ __forceinline__ uint32_t foldLane(uint32_t lane, uint32_t) const { return lane; }
	template <class LP, class Cnt>
	__device__ __forceinline__ void hit(const DScene &S, LP &lp, const Walk &w, AovStack &stk, Cnt &cnt, AovSample &s) const {
		const HitInfo h = finishHit<true, RARE>(S, lp.ro, lp.rd, w.hit, stk);
		const crh_material mat = loadMaterial(S, stk, h.material);
		ShadeRec rec;
		rec.dir = lp.rd; rec.point = h.point; rec.normal = h.normal; rec.uv = h.uv; rec.distance = w.hit.t; rec.ior = mat.ior;
		evalAlbedo(S, mat.bsdf, rec, cnt, stk, s.s0, s.s1, s.s2);
		if (!(RARE && w.hit.slot == -2)) { s.s3 = h.normal.x; s.s4 = h.normal.y; s.s5 = h.normal.z; }          /* (a scattering event's normal is a placeholder: zeros) */
		s.s6 = w.hit.t; s.s7 = 1.0f;
	}
	/* two 16-byte loads, renderer.c:288-291 channel by channel in pass order, two 16-byte stores */
	__device__ __forceinline__ void fold(size_t pixel, const lds_u32 *sp, uint32_t pc, int p0, uint32_t, uint32_t) const {
		f4 *const out = aov + pixel * 2u;
		f4 a = out[0], b = out[1];
		float unused = 0.0f;
		for (uint32_t k = 0; k < pc; ++k) {
			const int cs = p0 + (int)k + 1;
			foldSample(a.x, a.y, a.z, asF32(sp[k]), asF32(sp[CRH_BLOCK + k]), asF32(sp[2 * CRH_BLOCK + k]), cs);
			foldSample(a.w, b.x, b.y, asF32(sp[3 * CRH_BLOCK + k]), asF32(sp[4 * CRH_BLOCK + k]), asF32(sp[5 * CRH_BLOCK + k]), cs);
			foldSample(b.z, b.w, unused, asF32(sp[6 * CRH_BLOCK + k]), asF32(sp[7 * CRH_BLOCK + k]), 0.0f, cs);
		}
		out[0] = a; out[1] = b;
	}
};

/* SAMP: the sampler (0 random, 1 Halton); RARE: node programs or volumes, as in k_pathtrace_roll */
template <int SAMP, bool RARE>
__global__ __launch_bounds__(CRH_BLOCK, RARE ? 4 : CRH_AOV_WPS) void k_aov(const DScene Sarg, const crh_render_params P, const AovUnits U, float *aovArg, uint32_t rayFlags, uint32_t *ovfAll) {
	__shared__ uint32_t s_lane[CRH_AOV_LANE_WORDS * CRH_BLOCK];
	__shared__ __attribute__((aligned(16))) uint32_t s_inst0[CRH_AOV_INST_LDS ? CRH_INST_LDS0_MAX * 16u : 4u];
	CRH_EM_POW_TABLES_INIT();
	const DScene S = globalize(Sarg);
	AovStack stk = aovStack(S, s_lane, s_inst0, ovfAll);
	firstHitWaves(S, P, U, rayFlags, stk, AovKernel<SAMP, RARE>{(f4 *)(__attribute__((address_space(1))) f4 *)aovArg});
}
