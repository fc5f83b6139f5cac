/* ctx_buffers_check.cpp — test infrastructure: csrc/ctx_buffers.h (the owners of a context's per-dispatch buffers) on the HIP-on-CPU shim, whose allocations are
 * malloc and new: built with -fsanitize=address,undefined (tests/test_abi.py), every overrun, use after a growth, double free and leak of its types is an
 * error of this program — the leak check at exit is part of the assertion. */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <hip/hip_runtime.h>
#define HIP_TRY(expr) do { if ((expr) != hipSuccess) { std::printf("ctx_buffers_check: %s failed\n", #expr); return 1; } } while (0)
#include "../../c-ray_amd/csrc/ctx_buffers.h"

static int fail(const char *what) { std::printf("ctx_buffers_check: %s\n", what); return 1; }

static int deviceBuffer(hipStream_t stream) {
	DevBuf<uint32_t> b;
	if (b.grow(stream, 0) || b.p || b.n) return fail("DevBuf: a need of nothing allocated");
	if (b.grow(stream, 1000) || !b.p || b.n != 1000) return fail("DevBuf: growth from empty");
	for (size_t i = 0; i < b.n; ++i) b.p[i] = (uint32_t)i;
	uint32_t *const p0 = b.p;
	if (b.grow(stream, 1000) || b.grow(stream, 7) || b.p != p0 || b.n != 1000) return fail("DevBuf: a need that fits moved the block");
	if (b.p[999] != 999u) return fail("DevBuf: a need that fits touched the contents");
	if (b.grow(stream, 1001) || b.n != 1001) return fail("DevBuf: growth is not exact");
	for (size_t i = 0; i < b.n; ++i) b.p[i] = 0xA5A5A5A5u;
	b.release(); b.release();
	if (b.p || b.n) return fail("DevBuf: not empty after release");
	if (b.grow(stream, 3) || b.n != 3) return fail("DevBuf: growth after release");
	b.p[2] = 1u;
	b.release();
	return 0;
}

/* a write through the full capacity of both sides */
static void fill(StagedBuf &s, int v) { memset(s.dev, v, s.cap); memset(s.host, v, s.cap); }

static int stagedBuffer(hipStream_t stream) {
	StagedBuf never;
	never.release();                                   /* never reserved */
	StagedBuf s;
	if (s.reserve(1) || s.cap != 4096 || !s.dev || !s.host || !s.done) return fail("StagedBuf: the 4096-byte floor");
	fill(s, 1);
	void *const d0 = s.dev;
	if (s.reserve(4096) || s.dev != d0 || s.cap != 4096) return fail("StagedBuf: bytes that fit moved the block");
	fill(s, 5);
	if (s.reserve(4097) || s.cap != 2 * 4097) return fail("StagedBuf: 2 x bytes just above the capacity");
	fill(s, 2);
	if (s.reserve(2 * 4097 - 1) || s.cap != 2 * 4097) return fail("StagedBuf: just below the capacity");
	fill(s, 6);
	if (s.markInFlight(stream) || !s.inFlight) return fail("StagedBuf: markInFlight");
	if (s.reserve(100) || s.inFlight || s.cap != 2 * 4097) return fail("StagedBuf: reserve while in flight (bytes that fit)");
	fill(s, 7);
	if (s.markInFlight(stream) || s.reserve(20000) || s.inFlight || s.cap != 40000) return fail("StagedBuf: reserve while in flight (growth)");
	fill(s, 3);
	s.release();
	if (s.dev || s.host || s.done || s.cap || s.inFlight) return fail("StagedBuf: not empty after release");
	if (s.reserve(5000) || s.cap != 10000) return fail("StagedBuf: reserve after release");
	fill(s, 4);
	s.release(); s.release();
	return 0;
}

static int timedPairs(hipStream_t stream) {
	TimedPool pool;
	TimedPair a, b, c;
	if (pool.take(a) || pool.take(b) || !a.a || !a.b || !b.a || !b.b || a.a == b.a) return fail("TimedPool: two fresh pairs");
	HIP_TRY(hipEventRecord(a.a, stream));
	HIP_TRY(hipEventRecord(a.b, stream));
	float ms = -1.0f;
	HIP_TRY(hipEventElapsedTime(&ms, a.a, a.b));
	if (!(ms >= 0.0f)) return fail("TimedPool: the pair does not time");
	pool.give(a);
	if (pool.take(c) || c.a != a.a || c.b != a.b) return fail("TimedPool: take after give is not the same pair");
	pool.give(b); pool.give(c);
	if (pool.idle.size() != 2) return fail("TimedPool: pairs given back");
	pool.release();
	if (!pool.idle.empty()) return fail("TimedPool: not empty after release");
	pool.release();
	return 0;
}

/* what a dispatch path does with a pair: out of the pool, and back on every way out that does not keep it */
static int leased(TimedPool &pool, bool failEarly, bool keepIt, TimedPair &kept) {
	TimedLease lease(pool);
	if (lease.take()) return 1;
	if (failEarly) return 2;                           /* (a HIP_TRY between take and push) */
	if (keepIt) kept = lease.keep();
	return 0;
}

static int timedLease() {
	TimedPool pool;
	TimedPair kept;
	if (leased(pool, true, false, kept) != 2 || pool.idle.size() != 1) return fail("TimedLease: the pair of an early return is not back in the pool");
	const TimedPair first = pool.idle[0];
	if (leased(pool, false, false, kept) != 0 || pool.idle.size() != 1 || pool.idle[0].a != first.a) return fail("TimedLease: a lease that ends takes the pool's pair and gives it back");
	if (leased(pool, false, true, kept) != 0 || !pool.idle.empty() || kept.a != first.a || kept.b != first.b) return fail("TimedLease: a kept pair went back to the pool");
	pool.give(kept);
	pool.release();
	return 0;
}

/* a run of `laps` laps, complete or abandoned before stop() */
template <int LAPS> static int run(Stopwatch<LAPS> &w, hipStream_t stream, int laps, bool complete) {
	if (w.start(stream)) return 1;
	for (int i = 0; i < laps; ++i) if (w.mark(stream)) return 1;
	if (complete) w.stop();
	return 0;
}

static int stopwatch(hipStream_t stream) {
	constexpr int MAX = 5;
	Stopwatch<MAX> w;
	w.release();                                       /* never started */
	if (w.read() || w.laps != 0 || w.sum != 0.0f) return fail("Stopwatch: not zero laps and 0.0 before any run");
	if (run(w, stream, 1, true) || w.read() || w.laps != 1 || !(w.ms[0] >= 0.0f) || w.sum != w.ms[0]) return fail("Stopwatch: a run of one lap");
	if (run(w, stream, MAX, true)) return fail("Stopwatch: a run of the maximum number of laps");
	if (w.laps != 1) return fail("Stopwatch: a run changed the times before read()");
	if (w.mark(stream) == 0) return fail("Stopwatch: a lap beyond the last event");
	if (w.read() || w.laps != MAX) return fail("Stopwatch: reading the maximum number of laps");
	float sum = 0.0f, laps[MAX];
	for (int i = 0; i < MAX; ++i) { if (!(w.ms[i] >= 0.0f)) return fail("Stopwatch: a lap is negative"); laps[i] = w.ms[i]; sum += w.ms[i]; }
	if (sum != w.sum) return fail("Stopwatch: the sum is not the laps' float sum in launch order");
	if (w.read() || w.laps != MAX || w.sum != sum || memcmp(laps, w.ms, sizeof(laps))) return fail("Stopwatch: read() twice differs");
	if (run(w, stream, 2, false) || w.read() || w.laps != MAX || w.sum != sum || memcmp(laps, w.ms, sizeof(laps))) return fail("Stopwatch: a run that never stopped changed the times");
	/* what a creation that failed half-way leaves: some events, not all */
	HIP_TRY(hipEventDestroy(w.ev[2]));
	w.ev[2] = nullptr;
	hipEvent_t const e0 = w.ev[0];
	if (run(w, stream, 3, true) || !w.ev[2] || w.ev[0] != e0 || w.read() || w.laps != 3) return fail("Stopwatch: start() did not complete a partial set of events");
	const float sum3 = w.sum;
	w.release(); w.release();
	for (hipEvent_t e : w.ev) if (e) return fail("Stopwatch: an event after release");
	if (w.read() || w.laps != 3 || w.sum != sum3) return fail("Stopwatch: release lost the times");
	if (run(w, stream, 1, true) || w.read() || w.laps != 1) return fail("Stopwatch: a run after release");
	w.release();
	return 0;
}

int main() {
	hipStream_t stream = nullptr;
	HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
	if (deviceBuffer(stream) || stagedBuffer(stream) || timedPairs(stream) || timedLease() || stopwatch(stream)) return 1;
	HIP_TRY(hipStreamDestroy(stream));
	std::printf("ctx_buffers_check ok\n");
	return 0;
}
