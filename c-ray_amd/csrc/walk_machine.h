/*
 * walk_machine.h — the WALK-ONLY wave machine: what k_stream_walk (pathtrace_stream.h: the product's streaming form) and k_walk_probe form 3 (walk_probe.h: the measurement
 * that led to it) share, in one place. A wave walks rays — getClosestIsect, bvh.c:354-441 via pathtrace.c:26-30 — with the megakernel's lane code (walkBegin / stepNode /
 * stepTri / stepCtrl of pt_device.h) and its ballot scheduling, without path generation, shading, the job ring or the fold: lanes take rays from a RAY SOURCE as they fall
 * idle and leave the closest hit (t, u, v, prim slot | instance) in a global hit list. The two kernels differ in their ray source and in nothing else:
 *   WalkStack          the traversal stack of the walk-only kernels, walkStackPoint() to set it up
 *   stageInstLine0     line 0 of the instance records into the workgroup's LDS (k_aov stages the same lines for its own stack)
 *   walkRetireRefill   retire (write the hit record, go idle) + refill (the idle lanes take the source's next rays)
 *   walkOnlyMachine    the scheduling round: one loop body with one site per step kind
 * A ray source is a struct derived from WalkSource with two operations: fill() — called when the unit in hand is used up — sets cur / end to the next unit's slots or sets dry;
 * ray(i, o, d) gives origin and direction of slot i. Slot i's hit goes to hits[i] / hitInst[i].
 */
#pragma once

/* the walk kernels' traversal stack: NLDS entries in LDS (entry-major), deeper ones in the wave's overflow columns; the 15 park slots; line 0 of the instance records in LDS
 * when the scene has at most CRH_INST_LDS0_MAX instances (INST) */
template <int NLDS, bool INST>
struct WalkStack {
	lds_u32 *lds;
	lds_u32 *parkp;
	glb_u32 *ovf;
	const lds_u32 *inst0;
	__device__ __forceinline__ InstLine instLine(const DScene &S, int32_t idx, int line) const {
		if (INST && line == 0 && inst0) {
			const lds_u32 *p = inst0 + (uint32_t)idx * 16u;
			return InstLine{ldsLoadF4(p), ldsLoadF4(p + 4), ldsLoadF4(p + 8), ldsLoadF4(p + 12)};
		}
		const f4 *g = (const f4 *)(S.instances + idx) + 4 * line;
		return InstLine{g[0], g[1], g[2], g[3]};
	}
	__device__ __forceinline__ void park(int i, uint32_t v) { parkp[i * CRH_BLOCK] = v; }
	__device__ __forceinline__ uint32_t unpark(int i) { return parkp[i * CRH_BLOCK]; }
	__device__ __forceinline__ void push(uint32_t i, uint32_t v) {
		if (__builtin_expect(i < (uint32_t)NLDS, 1)) lds[i * CRH_BLOCK] = v;
		else ovf[(i - (uint32_t)NLDS) * 64u + (threadIdx.x & 63u)] = v;
	}
	__device__ __forceinline__ uint32_t pop(uint32_t i) {
		uint32_t v;
		if (__builtin_expect(i < (uint32_t)NLDS, 1)) v = lds[i * CRH_BLOCK];
		else v = ovf[(i - (uint32_t)NLDS) * 64u + (threadIdx.x & 63u)];
		return v;
	}
};

/* line 0 of the instance records into the workgroup's s_inst0 (scenes of <= CRH_INST_LDS0_MAX instances): the LDS copy, or null. Every thread of the workgroup calls it. */
template <size_t N>
__device__ __forceinline__ const lds_u32 *stageInstLine0(const DScene &S, uint32_t (&s_inst0)[N]) {
	if (S.instance_count > CRH_INST_LDS0_MAX) return nullptr;
	for (uint32_t i = threadIdx.x; i < S.instance_count * 16u; i += CRH_BLOCK) s_inst0[i] = ((const uint32_t *)(S.instances + (i >> 4)))[i & 15u];
	__syncthreads();
	return (const lds_u32 *)s_inst0;
}

/* this lane's columns of the workgroup's s_stack / s_park, and the wave's overflow columns */
template <int NLDS, bool INST>
__device__ __forceinline__ void walkStackPoint(WalkStack<NLDS, INST> &stk, uint32_t *s_stack, uint32_t *s_park, uint32_t *ovfAll) {
	const uint32_t wave = (blockIdx.x * CRH_BLOCK + threadIdx.x) >> 6;
	stk.lds = (lds_u32 *)&s_stack[threadIdx.x];
	stk.parkp = (lds_u32 *)&s_park[threadIdx.x];
	stk.ovf = (glb_u32 *)ovfAll + (size_t)__builtin_amdgcn_readfirstlane(wave) * CRH_OVF_WORDS_PER_WAVE;
}

/* what every ray source holds (wave-uniform) */
struct WalkSource {
	uint32_t cur = 0, end = 0;         /* the slots of the unit in hand whose rays have not started */
	bool dry = false;                  /* the source has no more units */
	__device__ __forceinline__ bool more() const { return !dry || cur != end; }
};

/* retire + refill (pathtrace_roll.h: retireRefill): lanes whose walk ended leave the hit in their slot's record; they and the idle lanes take the next rays of the unit in hand */
template <class Stk, class Cnt, class Port, class Src>
__device__ __forceinline__ void walkRetireRefill(const DScene &S, Walk &w, Stk &stk, Cnt &cnt, Port &port, const Sched &K, Src &src, f4 *hits, int32_t *hitInst, uint32_t &mySlot) {
	if (w.phase == PH_SHADE) {
		hits[mySlot] = f4{w.hit.t, w.hit.u, w.hit.v, asF32((uint32_t)w.hit.slot)};
		hitInst[mySlot] = w.hit.inst;
		w.phase = PH_IDLE;
	}
	const bool idle = (w.phase == PH_IDLE);
	const unsigned long long em = __ballot(idle);
	const uint32_t er = laneRank(em);
	if (src.cur == src.end && !src.dry) src.fill();
	const uint32_t take = min(src.end - src.cur, (uint32_t)__popcll(em));
	if (idle && er < take) {
		mySlot = src.cur + er;
		v3 o, d;
		src.ray(mySlot, o, d);
		walkBegin(S, w, stk, o, d, cnt, port, (uint32_t)K.rayFlags);
	}
	src.cur += take;
}

/* the machine: rounds until every lane is idle and the source is dry. `retireRefill` is the kernel's call of walkRetireRefill, `moreRays` its source's more(). */
template <class Stk, class Cnt, class Port, class Refill, class More>
__device__ __forceinline__ void walkOnlyMachine(const DScene &S, Walk &w, Stk &stk, Cnt &cnt, Port &port, const Sched &K, Refill &retireRefill, More &moreRays) {
	for (;;) {
		const uint32_t ph = w.phase;
		const int nN = __popcll(__ballot(ph == PH_NODE)), nT = __popcll(__ballot(ph == PH_TRI)), nC = __popcll(__ballot(ph == PH_CTRL || ph == PH_NODE_SLOW));
		const int nF = __popcll(__ballot(ph == PH_SHADE));
		const int nE = 64 - nN - nT - nC - nF;
		const int walkers = nN + nT + nC;
		const bool more = moreRays();
		if (walkers == 0 && nF == 0 && !more) break;
		/* the round picks a mode by the megakernel's rules — 0 a node run (which serves triangle, instance-entry and retire / refill steps in place once enough lanes wait
		 * for them), 1 a triangle run, 2 one control step, 3 retire + refill — and ONE loop body serves all four, so that the register allocator sees the largest step and not
		 * the sum of the copies that the round-level steps and the run's in-place steps inline (72 VGPRs; the megakernel's fused node run needs 126) */
		int mode = 0;
		if (walkers == 0 || (nF + nE >= K.swapMin && (nF > 0 || more))) mode = 3;
		else { int best = nN * K.wNode; if (nT * K.wTri > best) { best = nT * K.wTri; mode = 1; } if (nC * K.wCtrl > best) mode = 2; }
		const int n0 = mode == 1 ? nT : nN;
		bool again;
		do {
			if (mode == 0 && w.phase == PH_NODE) stepNode<true>(S, w, stk, cnt, port);
			const int nTw = (int)__popcll(__ballot(w.phase == PH_TRI));
			if (mode == 1 || (mode == 0 && nTw >= K.triInRun)) { if (w.phase == PH_TRI) stepTri(S, w, stk, cnt, port); }
			const int nCw = (int)__popcll(__ballot(w.phase == PH_CTRL));
			if (mode == 2 || (mode == 0 && nCw >= K.ctrlInRun)) {
				if (w.phase == PH_CTRL) stepCtrl(S, w, stk, cnt, port);
				if (mode == 2 && __ballot(w.phase == PH_NODE_SLOW)) { if (w.phase == PH_NODE_SLOW) stepNodeAny<false>(S, w, stk, cnt, port); }
			}
			const int nFi = (int)__popcll(__ballot(w.phase == PH_SHADE)), nEi = (int)__popcll(__ballot(w.phase == PH_IDLE));
			if (mode == 3 || (mode == 0 && nFi + nEi >= K.swapInRun && (nFi > 0 || moreRays()))) retireRefill();
			again = mode == 0 ? (int)__popcll(__ballot(w.phase == PH_NODE)) * 8 >= n0 * K.runNum : mode == 1 ? (int)__popcll(__ballot(w.phase == PH_TRI)) * 8 >= n0 * K.runNum : false;
		} while (again);
	}
}
