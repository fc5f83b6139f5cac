/*
 * exr_pack.h — k_pack_scanlines: the buffers the library already makes — the frame, the guide buffers, a denoised frame, ranked ids — gathered on the device into the
 * pixel-data section of an uncompressed scanline OpenEXR file whose channels are all FLOAT (crh_pack_scanlines, include/cray_hip.h): per stored row an int32 y, an int32
 * byte count, and then one plane of `width` 32-bit words per channel. The file format itself — header, offset table, Cryptomatte metadata — is the host's business
 * (c-ray_amd/host/exr_write.c, c-ray_amd/exr.py); nothing of the render path includes or calls anything in here.
 *
 * Shape. One lane per pixel of the chunk — a workgroup per stored row and 256 columns of it —, every lane runs the channel loop for its pixel: consecutive lanes write
 * consecutive words of a plane, so every store is coalesced, whatever the sources' strides are. The loads are strided (a lane's pixel is `stride` words from its
 * neighbour's): a wave's load of a stride-12 source touches 24 lines for 256 bytes it uses, and the same lines again for each of the source's other channels. Per-word
 * loads: a 16-byte load of a stride-8 or stride-12 pixel would hold words for channels that sit anywhere in the output order in registers across the loop, and the
 * descriptors say nothing about which channels share a pixel. The channel descriptors travel in the kernel's arguments (2 KB: wave-uniform scalar loads). No LDS, no
 * scratch, 416 bytes. One workgroup per whole row, its threads striding over x, takes the same time to the microsecond; with four channels in flight per
 * step that form was 1208 bytes, more than the library's size admits, and was not measured.
 *
 * A mapped channel holds ids as crh_ids_resolve writes them — (float)id, an empty rank -1 — and stores map[id]: the host's hash of the id's name; everything else —
 * negative, fractional, NaN, too large — stores 0.
 */
#pragma once

struct PackChan {
	const uint32_t *src;          /* [H, W, stride] words */
	const uint32_t *map;          /* device copy of the map, or null */
	uint32_t stride, component, mapCount, pad;
};
struct PackArgs { PackChan ch[CRH_PACK_MAX_CHANNELS]; };

/* the word a mapped channel stores for the source word w (the float is converted only once it is known to lie in [0, mapCount): exact, and the look-up in bounds) */
__device__ __forceinline__ uint32_t packMapped(const PackChan &k, uint32_t w) {
	const float v = __builtin_bit_cast(float, w);
	uint32_t out = 0u;
	if (v >= 0.0f && v < (float)k.mapCount) {
		const uint32_t u = (uint32_t)v;
		if ((float)u == v) out = asGlobal(k.map)[u];
	}
	return out;
}

/* out: gridDim.x blocks of 2 + nch * width words, block r the stored row firstRow + r; workgroup (r, j) packs the columns [j * CRH_BLOCK, (j + 1) * CRH_BLOCK) of it */
__global__ __launch_bounds__(CRH_BLOCK) void k_pack_scanlines(const PackArgs A, uint32_t nch, uint32_t width, uint32_t firstRow, uint32_t *outArg) {
	uint32_t *const out = (uint32_t *)(__attribute__((address_space(1))) uint32_t *)outArg;
	const uint32_t y = firstRow + blockIdx.x, x = blockIdx.y * CRH_BLOCK + threadIdx.x;
	uint32_t *const row = out + (size_t)blockIdx.x * (2u + (size_t)nch * width);
	if (x == 0) { row[0] = y; row[1] = 4u * nch * width; }
	if (x >= width) return;
	const size_t pixel = (size_t)y * width + x;
	for (uint32_t c = 0; c < nch; ++c) {
		const PackChan k = A.ch[c];
		uint32_t w = asGlobal(k.src)[pixel * k.stride + k.component];
		if (k.map) w = packMapped(k, w);
		row[2u + c * width + x] = w;          /* (nch * width < 2^29: crh_pack_scanlines) */
	}
}
