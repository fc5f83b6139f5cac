/*
 * half_check.cpp — TEST INFRASTRUCTURE: exr_zip.h's zipHalfBits() (binary32 -> binary16 in integer arithmetic, the rule of include/cray_hip_exr.h) on the host.
 *   half_check                 all 2^32 words: every non-NaN input against the CPU's F16C conversion (_cvtss_sh, round to nearest), every NaN against the rule,
 *                              stated here a second time; at most 16 threads
 *   half_check <in> <out>      the conversions of the little-endian 32-bit words of file <in> as 16-bit words into file <out> (for a comparison with numpy)
 * Exit 0: no mismatch; 1: mismatches; 77: the CPU has no F16C.
 */
#include <immintrin.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
#define CRX_ZIP_CONVERSION_ONLY
#include "../../c-ray_amd/csrc/exr_zip.h"

/* the NaN rule, restated: the sign, an all-ones exponent, the top ten mantissa bits — and bit 0 where those ten are zero, so that a NaN stays one */
static uint32_t nanRule(uint32_t w) {
	uint32_t h = ((w >> 31) << 15) | 0x7c00u | ((w & 0x007fffffu) >> 13);
	if ((h & 0x03ffu) == 0u) h |= 1u;
	return h;
}

int main(int argc, char **argv) {
	if (argc == 3) {
		FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
		if (!in || !out) return 2;
		std::vector<uint32_t> words(1u << 16);
		std::vector<uint16_t> halves(1u << 16);
		size_t n;
		while ((n = fread(words.data(), 4, words.size(), in)) > 0) {
			for (size_t i = 0; i < n; ++i) halves[i] = (uint16_t)zipHalfBits(words[i]);
			if (fwrite(halves.data(), 2, n, out) != n) return 2;
		}
		fclose(in);
		return fclose(out) ? 2 : 0;
	}
	if (!__builtin_cpu_supports("f16c")) { printf("half_check: this CPU has no F16C\n"); return 77; }
	uint64_t bad = 0, n = 0, nans = 0;
	uint32_t firstBad = 0;
	#pragma omp parallel for reduction(+ : bad, n, nans) schedule(static) num_threads(16)
	for (int64_t block = 0; block < 1 << 16; ++block) {
		for (uint32_t low = 0; low < 1u << 16; ++low) {
			const uint32_t w = (uint32_t)block << 16 | low;
			const uint32_t got = zipHalfBits(w);
			uint32_t want;
			if ((w & 0x7fffffffu) > 0x7f800000u) { want = nanRule(w); ++nans; }
			else {
				float x;
				memcpy(&x, &w, 4);
				want = (uint32_t)_cvtss_sh(x, _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC) & 0xffffu;
			}
			++n;
			if (got != want || got > 0xffffu) {
				++bad;
				#pragma omp critical
				firstBad = w;
			}
		}
	}
	printf("half tested %llu (NaNs %llu) mismatches %llu", (unsigned long long)n, (unsigned long long)nans, (unsigned long long)bad);
	if (bad) printf(" (one of them: %08x)", firstBad);
	printf("\n");
	return bad ? 1 : 0;
}
