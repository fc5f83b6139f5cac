/*
 * exr_zip_emu.cpp — libcray_hip_exr_emu.so: c-ray_amd/csrc/exr_zip.hip (the companion library's kernels AND its C-ABI host code, unmodified) compiled for the host
 * against the HIP-on-CPU shim in hipemu/. TEST INFRASTRUCTURE ONLY (Makefile.exr): the CPU-only tier runs tests/test_exr_zip.py's GPU tests through it. Never loaded
 * by the product, bench.py or the GPU tests.
 */
#include "../../c-ray_amd/csrc/exr_zip.hip"

extern "C" {
/* emulation bookkeeping: {kernel launches, blocks, wave collectives resolved, lane switches}; its presence is how a binding recognises the emulation */
void crx_emu_stats(uint64_t out[4]) {
	const hipemu::Stats s = hipemu::stats();
	out[0] = s.launches; out[1] = s.blocks; out[2] = s.collectives; out[3] = s.switches;
}
}
