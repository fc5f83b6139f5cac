/*
 * ctx_buffers.h — who owns a context's per-dispatch device memory (cray_hip.hip: crh_ctx). Three idioms of the host code, each said once:
 *   DevBuf<T>    a grow-only device array: "grow this buffer if the dispatch needs more";
 *   StagedBuf    a device buffer with a pinned host twin, a `done` event and an in-flight flag: the per-dispatch list staging (tile lists, the adaptive step's results);
 *   TimedPool    the {a, b} event pairs around a timed kernel (crh_kernel_time_ms), taken from a pool and given back — by a TimedLease on every path that does not keep them;
 *   Stopwatch    up to LAPS laps on a stream, read later: the events around the launches of an entry point that has one run in flight at a time (AOV, denoise, adaptive).
 * HIP runtime API only — nothing of the context, the scene or the kernels. The includer defines HIP_TRY(expr) first: it returns a non-zero int from the enclosing
 * function when expr is not hipSuccess (cray_hip.hip's sets crh_last_error; tests/emu/ctx_buffers_check.cpp includes this file over the HIP-on-CPU shim).
 * Every function that can fail returns 0 (CRH_OK) or what HIP_TRY returned. release() is explicit: a context is torn down under hipSetDevice, behind a stream drain,
 * by crh_context_destroy — not by destructors, wherever the object happens to die.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <vector>

#ifndef HIP_TRY
#error "ctx_buffers.h: define HIP_TRY(expr) before including this file"
#endif

/* `n` elements at `p`, or nothing. Contents do not survive a growth (no caller needs them to). */
template <class T> struct DevBuf {
	T *p = nullptr;
	size_t n = 0;
	/* at least `need` elements: nothing to do if they are there; otherwise the stream is drained (work in flight may still read the old block), the old block
	 * freed and exactly `need` allocated. On any failure the buffer is empty: p null, n zero. */
	int grow(hipStream_t stream, size_t need) {
		if (need <= n) return 0;
		HIP_TRY(hipStreamSynchronize(stream));
		T *const old = p;
		p = nullptr; n = 0;
		if (old) HIP_TRY(hipFree(old));
		void *fresh = nullptr;
		HIP_TRY(hipMalloc(&fresh, need * sizeof(T)));
		p = (T *)fresh; n = need;
		return 0;
	}
	void release() {
		if (p) (void)hipFree(p);
		p = nullptr; n = 0;
	}
};

/* `cap` bytes on the device and as many of pinned host memory. The user fills `host`, puts its copy (or a kernel that reads `host` through its mapped address) and the
 * consumer on a stream, and marks the buffer in flight; the next reserve() waits for that consumer before the bytes are touched again. Which way the bytes travel,
 * and what else sits on the stream around them, is the caller's business. */
struct StagedBuf {
	void *dev = nullptr, *host = nullptr;
	size_t cap = 0;
	hipEvent_t done = nullptr;          /* recorded behind the last consumer (timing disabled); created by the first reserve() */
	bool inFlight = false;
	/* room for `bytes` on both sides, free to be written: waits for the consumer in flight, and regrows both sides to max(4096, 2 x bytes) if bytes do not fit */
	int reserve(size_t bytes) {
		if (inFlight) { HIP_TRY(hipEventSynchronize(done)); inFlight = false; }
		if (bytes > cap) {
			void *const d = dev, *const h = host;
			dev = host = nullptr; cap = 0;
			if (d) HIP_TRY(hipFree(d));
			if (h) HIP_TRY(hipHostFree(h));
			const size_t want = std::max<size_t>(4096, 2 * bytes);
			HIP_TRY(hipMalloc(&dev, want));
			HIP_TRY(hipHostMalloc(&host, want, hipHostMallocDefault));
			cap = want;
		}
		if (!done) HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
		return 0;
	}
	int markInFlight(hipStream_t stream) {
		HIP_TRY(hipEventRecord(done, stream));
		inFlight = true;
		return 0;
	}
	void release() {
		if (dev) (void)hipFree(dev);
		if (host) (void)hipHostFree(host);
		if (done) (void)hipEventDestroy(done);
		dev = host = nullptr; cap = 0; done = nullptr; inFlight = false;
	}
};

struct TimedPair { hipEvent_t a = nullptr, b = nullptr; };
struct TimedPool {
	std::vector<TimedPair> idle;
	int take(TimedPair &ev) {
		if (!idle.empty()) { ev = idle.back(); idle.pop_back(); return 0; }
		HIP_TRY(hipEventCreate(&ev.a));
		HIP_TRY(hipEventCreate(&ev.b));
		return 0;
	}
	void give(const TimedPair &ev) { idle.push_back(ev); }
	void release() {
		for (const TimedPair &t : idle) { if (t.a) (void)hipEventDestroy(t.a); if (t.b) (void)hipEventDestroy(t.b); }
		idle.clear();
	}
};
/* A pair out of the pool for the length of a scope: whoever leaves the scope without keep() — every early return — gives the pair back. */
struct TimedLease {
	TimedPool &pool;
	TimedPair ev;
	bool held = false;
	explicit TimedLease(TimedPool &p) : pool(p) {}
	TimedLease(const TimedLease &) = delete;
	TimedLease &operator=(const TimedLease &) = delete;
	~TimedLease() { if (held) pool.give(ev); }
	int take() {
		const int rc = pool.take(ev);
		held = rc == 0;
		return rc;
	}
	/* the pair is the caller's now (the render path queues it until its times are read) */
	TimedPair keep() { held = false; return ev; }
};

/* Up to LAPS laps between LAPS + 1 timing events on a stream: start(), a mark() behind every timed launch, stop() once the run is complete; read() waits for a
 * complete run once and keeps its times — `laps` of them in `ms`, summed in launch order in `sum`. A run that never reached stop() (a launch failed in between)
 * is no run: the times stay those of the last complete one, and zero laps / 0.0 before the first. */
template <int LAPS> struct Stopwatch {
	hipEvent_t ev[LAPS + 1] = {};
	int marks = 0;                      /* laps recorded since start() */
	bool fresh = false;                 /* a complete run that read() has not taken yet */
	int laps = 0;
	float ms[LAPS] = {};
	float sum = 0.0f;
	int start(hipStream_t stream) {
		fresh = false; marks = 0;
		for (hipEvent_t &e : ev) if (!e) HIP_TRY(hipEventCreate(&e));
		HIP_TRY(hipEventRecord(ev[0], stream));
		return 0;
	}
	int mark(hipStream_t stream) {
		HIP_TRY(marks < LAPS ? hipSuccess : hipErrorInvalidValue);
		HIP_TRY(hipEventRecord(ev[marks + 1], stream));
		++marks;
		return 0;
	}
	void stop() { fresh = marks > 0; }
	int read() {
		if (!fresh) return 0;
		HIP_TRY(hipEventSynchronize(ev[marks]));
		float lap[LAPS], total = 0.0f;
		for (int i = 0; i < marks; ++i) {
			HIP_TRY(hipEventElapsedTime(&lap[i], ev[i], ev[i + 1]));
			total += lap[i];
		}
		std::copy(lap, lap + marks, ms);
		laps = marks; sum = total; fresh = false;
		return 0;
	}
	void release() {
		for (hipEvent_t &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
		marks = 0; fresh = false;
	}
};
