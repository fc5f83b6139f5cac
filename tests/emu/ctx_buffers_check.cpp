/* ctx_buffers_check.cpp — test infrastructure: csrc/ctx_buffers.h (the owners of a context's per-dispatch buffers) on the HIP-on-CPU shim, whose allocations are
 * malloc and new: built with -fsanitize=address,undefined (tests/test_abi.py), every overrun, use after a growth, double free and leak of the three types is an
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

int main() {
	hipStream_t stream = nullptr;
	HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
	if (deviceBuffer(stream) || stagedBuffer(stream) || timedPairs(stream)) return 1;
	HIP_TRY(hipStreamDestroy(stream));
	std::printf("ctx_buffers_check ok\n");
	return 0;
}
