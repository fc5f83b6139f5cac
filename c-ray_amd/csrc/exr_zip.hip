/*
 * exr_zip.hip — libcray_hip_exr.so: the C-ABI of include/cray_hip_exr.h around the kernels of exr_zip.h (the layers file's chunks) and of png_pack.h (the 8-bit
 * frame as a PNG, which shares exr_zip.h's deflate and, through srgb8.h, the product's float-to-byte rule; png_display.h beside it: the display transform and the
 * automatic exposure; despeckle.h: the firefly filter, which is no codec but needs no scene either). A translation unit of its own: it shares no state with
 * libcray_hip.so and includes of it only what is plain HIP runtime bookkeeping (ctx_buffers.h: DevBuf, Stopwatch) and the channel descriptor (cray_hip.h).
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "cray_hip_exr.h"

namespace {
thread_local std::string g_error;
int fail(int code, const std::string &what) { g_error = what; return code; }
}  // namespace
#define HIP_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(CRH_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); } while (0)
#include "ctx_buffers.h"
#include "exr_zip.h"
#include "png_pack.h"
#include "despeckle.h"

struct crx_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	bool ownStream = false;
	DevBuf<uint32_t> dT, dSegOut, dMeta, dMaps;          /* T' of every chunk; the segments' outputs; segMeta + segOff + chunkInfo; the id maps of the call */
	DevBuf<uint64_t> dPos;                               /* chunkPos */
	DevBuf<uint8_t> dOut;                                /* the compacted result */
	void *pinned = nullptr;
	size_t pinnedBytes = 0;
	Stopwatch<CRX_ZIP_PHASES> watch;
	DevBuf<uint32_t> dImg;                               /* crx_png_pack: the 8-bit image, in words */
	DevBuf<uint8_t> dTypes;                              /* ... and every row's filter type */
	Stopwatch<CRX_PNG_PHASES> pngWatch;
	DevBuf<uint32_t> dHist;                              /* crx_auto_exposure: the CRX_HIST_BINS bins, then k_png_pick's four result words */
	Stopwatch<1> autoWatch;
	DevBuf<uint32_t> dScale;                             /* crx_despeckle: the scale plane, rounded up to four floats, then the four stats words */
	int scaleWidth = 0, scaleHeight = 0;                 /* ... of the last complete call; 0 before it */
	Stopwatch<2> despeckleWatch;
	int codes = CRX_CODES_FIXED;                         /* crx_set_codes */
};

namespace {
int growPinned(crx_ctx *c, size_t bytes) {
	if (bytes <= c->pinnedBytes) return 0;
	HIP_TRY(hipStreamSynchronize(c->stream));
	void *const old = c->pinned;
	c->pinned = nullptr; c->pinnedBytes = 0;
	if (old) HIP_TRY(hipHostFree(old));
	HIP_TRY(hipHostMalloc(&c->pinned, bytes, hipHostMallocDefault));
	c->pinnedBytes = bytes;
	return 0;
}
}  // namespace

extern "C" {

const char *crx_last_error(void) { return g_error.c_str(); }
uint32_t crx_zip_segment_bytes(void) { return CRX_SEG; }

int crx_context_create(int device, void *stream, crx_ctx **out) {
	if (!out) return fail(CRH_ERR_INVALID, "crx_context_create: out is NULL");
	*out = nullptr;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count < 1) { (void)hipGetLastError(); return fail(CRH_ERR_NO_DEVICE, "crx_context_create: no HIP device (there is no CPU path)"); }
	if (device < 0 || device >= count) return fail(CRH_ERR_INVALID, "crx_context_create: no such device");
	HIP_TRY(hipSetDevice(device));
	crx_ctx *const c = new crx_ctx;
	c->device = device;
	if (stream) c->stream = (hipStream_t)stream;
	else {
		const hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
		if (e != hipSuccess) { delete c; return fail(CRH_ERR_HIP, std::string("crx_context_create: ") + hipGetErrorString(e)); }
		c->ownStream = true;
	}
	*out = c;
	return CRH_OK;
}

int crx_context_destroy(crx_ctx *c) {
	if (!c) return CRH_OK;
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	c->dT.release(); c->dSegOut.release(); c->dMeta.release(); c->dMaps.release(); c->dPos.release(); c->dOut.release();
	if (c->pinned) (void)hipHostFree(c->pinned);
	c->watch.release();
	c->dImg.release(); c->dTypes.release(); c->pngWatch.release();
	c->dHist.release(); c->autoWatch.release();
	c->dScale.release(); c->despeckleWatch.release();
	if (c->ownStream) (void)hipStreamDestroy(c->stream);
	delete c;
	return CRH_OK;
}

}  // extern "C"

namespace {
/* crx_pack_zip (types NULL, allRaw false) and crx_pack. A call without a HALF channel launches k_zip_transform and k_zip_emit, as it always has. */
int pack(const char *who, crx_ctx *c, const crh_pack_channel *ch, const uint8_t *types, uint32_t nch, int width, int height, int first_row, int row_count, int lines_per_chunk,
         bool allRaw, void *host_out, uint64_t *chunk_bytes_host, uint64_t *total_bytes) {
	bool ok = c && ch && host_out && chunk_bytes_host && total_bytes && nch >= 1 && nch <= CRH_PACK_MAX_CHANNELS && width > 0 && height > 0 && first_row >= 0 &&
	          row_count >= 0 && row_count <= height - first_row && (uint64_t)nch * (uint64_t)width < (1ull << 29) - 2u && (lines_per_chunk == 1 || lines_per_chunk == 16);
	ok = ok && first_row % lines_per_chunk == 0 && (first_row + row_count == height || (first_row + row_count) % lines_per_chunk == 0);
	ZipArgs A;
	ZipRow R;
	memset(&A, 0, sizeof(A));
	memset(&R, 0, sizeof(R));
	size_t mapAt[CRH_PACK_MAX_CHANNELS], mapWords = 0;          /* channels that name the same map share its copy; the first of them in the list (bit i) uploads it */
	uint64_t first = 0;
	bool mixed = false;
	for (uint32_t i = 0; ok && i < nch; ++i) {
		const crh_pack_channel &k = ch[i];
		const uint32_t type = types ? types[i] : (uint32_t)CRX_PIXEL_FLOAT;
		ok = k.dev_src && k.stride >= 1 && k.stride <= 64 && k.component < k.stride && k.map_count <= 65536 && (!k.map_host || k.map_count) &&
		     (type == CRX_PIXEL_FLOAT || (type == CRX_PIXEL_HALF && !k.map_host));
		A.ch[i] = ZipChan{(const uint32_t *)k.dev_src, k.map_host, k.stride, k.component, k.map_count, type == CRX_PIXEL_HALF ? 1u : 0u};
		R.off[i + 1u] = R.off[i] + (type == CRX_PIXEL_HALF ? 2u : 4u) * (uint32_t)width;          /* (< 2^31: nch * width < 2^29) */
		mixed = mixed || type == CRX_PIXEL_HALF;
		uint32_t j = 0;
		while (j < i && (ch[j].map_host != k.map_host || ch[j].map_count != k.map_count)) ++j;
		mapAt[i] = j < i ? mapAt[j] : mapWords;
		if (j == i && k.map_host) { first |= 1ull << i; mapWords += k.map_count; }
	}
	ok = ok && (uint64_t)R.off[nch] * (uint64_t)lines_per_chunk < (1ull << 31);
	if (!ok) return fail(CRH_ERR_INVALID, std::string(who) + ": bad argument");
	if (row_count == 0) { *total_bytes = 0; return CRH_OK; }

	ZipGeom G;
	G.nch = nch; G.width = (uint32_t)width; G.firstRow = (uint32_t)first_row; G.rowCount = (uint32_t)row_count; G.lpc = (uint32_t)lines_per_chunk;
	G.nchunks = (G.rowCount + G.lpc - 1u) / G.lpc;
	G.rowBytes = R.off[nch];
	G.fullBytes = G.rowBytes * G.lpc;
	G.pitch = (G.fullBytes + 3u) / 4u;
	G.allRaw = allRaw ? 1u : 0u;
	G.segsPerChunk = (G.fullBytes + CRX_SEG - 1u) / CRX_SEG;
	const uint32_t blocksPerChunk = (G.pitch + 255u) / 256u;
	const uint64_t segs = (uint64_t)G.nchunks * G.segsPerChunk, blocks = (uint64_t)G.nchunks * blocksPerChunk;
	if (segs >= (1ull << 31) || blocks >= (1ull << 31)) return fail(CRH_ERR_NOMEM, std::string(who) + ": too many rows for one call (pass fewer rows at a time)");
	const size_t rawBytes = (size_t)G.rowBytes * (size_t)row_count, outBytes = 8u * (size_t)G.nchunks + rawBytes;
	const size_t sizeWords = 2u * (size_t)G.nchunks + 1u;          /* chunkPos */

	HIP_TRY(hipSetDevice(c->device));
	int rc;
	if ((rc = c->dT.grow(c->stream, allRaw ? 1u : (size_t)G.nchunks * G.pitch))) return rc;
	if ((rc = c->dSegOut.grow(c->stream, allRaw ? 1u : (size_t)segs * (CRX_SEG_OUT / 4u)))) return rc;
	if ((rc = c->dMeta.grow(c->stream, 5u * (size_t)segs + 4u * (size_t)G.nchunks))) return rc;
	if ((rc = c->dMaps.grow(c->stream, mapWords ? mapWords : 1u))) return rc;
	if ((rc = c->dPos.grow(c->stream, sizeWords))) return rc;
	if ((rc = c->dOut.grow(c->stream, outBytes))) return rc;
	if ((rc = growPinned(c, outBytes > sizeWords * 8u ? outBytes : sizeWords * 8u))) return rc;
	uint32_t *const segMeta = c->dMeta.p, *const segOff = segMeta + 4u * (size_t)segs, *const chunkInfo = segOff + (size_t)segs;

	for (uint32_t i = 0; i < nch; ++i) {
		if (!A.ch[i].map) continue;
		uint32_t *const dev = c->dMaps.p + mapAt[i];
		if (first >> i & 1u) HIP_TRY(hipMemcpyAsync(dev, A.ch[i].map, A.ch[i].mapCount * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		A.ch[i].map = dev;
	}
	if ((rc = c->watch.start(c->stream))) return rc;
	if (!allRaw) {
		if (mixed) hipLaunchKernelGGL(k_zip_transform_mixed, dim3((uint32_t)blocks), dim3(256), 0, c->stream, A, R, G, blocksPerChunk, c->dT.p);
		else hipLaunchKernelGGL(k_zip_transform, dim3((uint32_t)blocks), dim3(256), 0, c->stream, A, G, blocksPerChunk, c->dT.p);
		HIP_TRY(hipGetLastError());
	}
	if ((rc = c->watch.mark(c->stream))) return rc;
	if (!allRaw) {
		if (c->codes == CRX_CODES_DYNAMIC) hipLaunchKernelGGL(k_zip_deflate_dynamic, dim3((uint32_t)segs), dim3(64), 0, c->stream, G, c->dT.p, c->dSegOut.p, segMeta);
		else hipLaunchKernelGGL(k_zip_deflate, dim3((uint32_t)segs), dim3(64), 0, c->stream, G, c->dT.p, c->dSegOut.p, segMeta);
		HIP_TRY(hipGetLastError());
	}
	if ((rc = c->watch.mark(c->stream))) return rc;
	hipLaunchKernelGGL(k_zip_scan, dim3(1), dim3(256), 0, c->stream, G, segMeta, segOff, chunkInfo, c->dPos.p);
	HIP_TRY(hipGetLastError());
	if ((rc = c->watch.mark(c->stream))) return rc;
	if (mixed) hipLaunchKernelGGL(k_zip_emit_mixed, dim3((uint32_t)segs), dim3(256), 0, c->stream, A, R, G, c->dSegOut.p, segMeta, segOff, chunkInfo, c->dPos.p, c->dOut.p);
	else hipLaunchKernelGGL(k_zip_emit, dim3((uint32_t)segs), dim3(256), 0, c->stream, A, G, c->dSegOut.p, segMeta, segOff, chunkInfo, c->dPos.p, c->dOut.p);
	HIP_TRY(hipGetLastError());
	if ((rc = c->watch.mark(c->stream))) return rc;
	c->watch.stop();

	/* the sizes first: they say how many bytes to fetch */
	uint64_t *const sizes = (uint64_t *)c->pinned;
	HIP_TRY(hipMemcpyAsync(sizes, c->dPos.p, sizeWords * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint64_t total = sizes[2u * (size_t)G.nchunks];
	if (total > outBytes || total < 8u * (uint64_t)G.nchunks) return fail(CRH_ERR_HIP, std::string(who) + ": the device reported an impossible size");
	memcpy(chunk_bytes_host, sizes + G.nchunks, G.nchunks * sizeof(uint64_t));
	*total_bytes = total;
	HIP_TRY(hipMemcpyAsync(c->pinned, c->dOut.p, total, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	memcpy(host_out, c->pinned, total);
	return CRH_OK;
}
}  // namespace

extern "C" {

int crx_pack_zip(crx_ctx *c, const crh_pack_channel *ch, uint32_t nch, int width, int height, int first_row, int row_count, int lines_per_chunk, void *host_out,
                 uint64_t *chunk_bytes_host, uint64_t *total_bytes) {
	return pack("crx_pack_zip", c, ch, nullptr, nch, width, height, first_row, row_count, lines_per_chunk, false, host_out, chunk_bytes_host, total_bytes);
}

int crx_pack(crx_ctx *c, const crh_pack_channel *ch, const uint8_t *pixel_types, uint32_t nch, int width, int height, int first_row, int row_count, int compression,
             void *host_out, uint64_t *chunk_bytes_host, uint64_t *total_bytes) {
	if (compression != 0 && compression != 2 && compression != 3) return fail(CRH_ERR_INVALID, "crx_pack: bad argument (compression is 0, 2 or 3)");
	return pack("crx_pack", c, ch, pixel_types, nch, width, height, first_row, row_count, compression == 3 ? 16 : 1, compression == 0, host_out, chunk_bytes_host, total_bytes);
}

int crx_set_codes(crx_ctx *c, int codes) {
	if (!c || (codes != CRX_CODES_FIXED && codes != CRX_CODES_DYNAMIC)) return fail(CRH_ERR_INVALID, "crx_set_codes: bad argument (a context, and CRX_CODES_FIXED or CRX_CODES_DYNAMIC)");
	c->codes = codes;
	return CRH_OK;
}

int crx_get_codes(crx_ctx *c, int *codes) {
	if (!c || !codes) return fail(CRH_ERR_INVALID, "crx_get_codes: NULL argument");
	*codes = c->codes;
	return CRH_OK;
}

int crx_debug_code_lengths(crx_ctx *c, const uint32_t *freq, uint32_t symbols, uint32_t limit, uint32_t count, uint8_t *lengths) {
	bool ok = c && freq && lengths && symbols >= 1 && symbols <= CRX_MAX_SYMBOLS && (limit == 7 || limit == 15) && symbols <= (1u << limit) && count < (1u << 20);
	for (uint32_t h = 0; ok && h < count; ++h) {
		uint64_t sum = 0;
		for (uint32_t s = 0; s < symbols; ++s) sum += freq[(size_t)h * symbols + s];
		ok = sum < CRX_FREQ_LIMIT;
	}
	if (!ok) return fail(CRH_ERR_INVALID, "crx_debug_code_lengths: bad argument");
	if (count == 0) return CRH_OK;
	const size_t n = (size_t)count * symbols;
	HIP_TRY(hipSetDevice(c->device));
	int rc;
	if ((rc = c->dT.grow(c->stream, n))) return rc;
	if ((rc = c->dOut.grow(c->stream, n))) return rc;
	HIP_TRY(hipMemcpyAsync(c->dT.p, freq, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_zip_code_lengths, dim3(count), dim3(64), 0, c->stream, c->dT.p, symbols, limit, c->dOut.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(lengths, c->dOut.p, n, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return CRH_OK;
}

int crx_pack_zip_phases_ms(crx_ctx *c, float phases_ms[CRX_ZIP_PHASES]) {
	if (!c || !phases_ms) return fail(CRH_ERR_INVALID, "crx_pack_zip_phases_ms: NULL argument");
	HIP_TRY(hipSetDevice(c->device));
	const int rc = c->watch.read();
	if (rc) return rc;
	for (int i = 0; i < CRX_ZIP_PHASES; ++i) phases_ms[i] = i < c->watch.laps ? c->watch.ms[i] : 0.0f;
	return CRH_OK;
}

int crx_pack_zip_time_ms(crx_ctx *c, float *ms) {
	float phases[CRX_ZIP_PHASES];
	if (!ms) return fail(CRH_ERR_INVALID, "crx_pack_zip_time_ms: NULL argument");
	const int rc = crx_pack_zip_phases_ms(c, phases);
	if (rc) return rc;
	*ms = c->watch.sum;
	return CRH_OK;
}

}  // extern "C"

/* ---- the PNG codec (png_pack.h) ---- */
namespace {
void pngPut4(std::string &s, uint32_t v) { const char b[4] = {(char)(v >> 24), (char)(v >> 16), (char)(v >> 8), (char)v}; s.append(b, 4); }
/* a chunk: length, type, data, the CRC-32 of type and data (pngCrcByte: the device's own step, conditioned here) */
void pngChunk(std::string &s, const char *type, const std::string &data) {
	pngPut4(s, (uint32_t)data.size());
	const size_t at = s.size();
	s.append(type, 4);
	s += data;
	uint32_t r = 0xffffffffu;
	for (size_t i = at; i < s.size(); ++i) r = pngCrcByte(r, (uint8_t)s[i]);
	pngPut4(s, ~r);
}
/* what the arguments make of the file: n bytes of filtered data, and — with `head` — everything up to and including the zlib header, the IDAT's length left 0.
 * False: an argument crx_png_bound and crx_png_pack refuse. */
bool pngLayout(int width, int height, const crx_png_text *text, uint32_t text_count, uint64_t *n, uint64_t *headBytes, std::string *head) {
	if (width <= 0 || height <= 0 || (text_count && !text)) return false;
	*n = (3u * (uint64_t)width + 1u) * (uint64_t)height;
	if (*n >= (1ull << 31)) return false;
	uint64_t bytes = 8u + 25u;
	for (uint32_t i = 0; i < text_count; ++i) {
		if (!text[i].key || !text[i].value) return false;
		const size_t k = strlen(text[i].key), v = strlen(text[i].value);
		if (k < 1 || k > 79 || v >= (1ull << 31) - 80u) return false;
		bytes += 12u + k + 1u + v;
	}
	*headBytes = bytes + 8u + 2u;
	if (*headBytes >= (1ull << 31)) return false;
	if (!head) return true;
	head->assign("\x89PNG\r\n\x1a\n", 8);
	std::string ihdr;
	pngPut4(ihdr, (uint32_t)width); pngPut4(ihdr, (uint32_t)height);
	ihdr.append("\x08\x02\x00\x00\x00", 5);          /* 8 bits a sample, colour type 2 (RGB), deflate, the five filters, no interlace */
	pngChunk(*head, "IHDR", ihdr);
	for (uint32_t i = 0; i < text_count; ++i) pngChunk(*head, "tEXt", std::string(text[i].key) + '\0' + text[i].value);
	pngPut4(*head, 0u);
	head->append("IDAT\x78\x01", 6);
	return head->size() == *headBytes;
}
uint64_t pngBound(uint64_t n, uint64_t headBytes) { return headBytes + (n + CRX_SEG - 1u) / CRX_SEG * CRX_SEG_OUT + CRX_PNG_FIXED_TAIL; }
}  // namespace

extern "C" {

int crx_png_bound(int width, int height, const crx_png_text *text, uint32_t text_count, uint64_t *bytes) {
	uint64_t n = 0, headBytes = 0;
	if (!bytes || !pngLayout(width, height, text, text_count, &n, &headBytes, nullptr)) return fail(CRH_ERR_INVALID, "crx_png_bound: bad argument");
	*bytes = pngBound(n, headBytes);
	return CRH_OK;
}

}  // extern "C"

namespace {
bool displayValid(const crx_display &d) {
	return d.curve >= CRX_CURVE_CLAMP && d.curve <= CRX_CURVE_HABLE && d.exposure >= CRX_EXPOSURE_MIN && d.exposure <= CRX_EXPOSURE_MAX && d.white >= CRX_WHITE_MIN &&
	       d.white <= CRX_WHITE_MAX && (d.dither == 0 || d.dither == 1);          /* (a NaN fails every comparison) */
}
bool displayIdentity(const crx_display &d) { return d.exposure == 1.0f && d.curve == CRX_CURVE_CLAMP && d.dither == 0; }

/* crx_png_pack (display NULL) and crx_png_pack_display: one body, the convert launch apart. The identity launches k_png_convert, as crx_png_pack always has. */
int pngPack(const char *who, crx_ctx *c, const float *dev_fb, int width, int height, const crx_display *display, int filter, const crx_png_text *text, uint32_t text_count,
            void *host_out, uint64_t capacity, uint64_t *total_bytes) {
	uint64_t n64 = 0, headBytes = 0;
	std::string head;
	if (!c || !dev_fb || !host_out || !total_bytes || filter < CRX_PNG_FILTER_ADAPTIVE || filter > 4 || (display && !displayValid(*display)) ||
	    !pngLayout(width, height, text, text_count, &n64, &headBytes, &head) || capacity < pngBound(n64, headBytes))
		return fail(CRH_ERR_INVALID, std::string(who) + ": bad argument (a context, a frame, an output of crx_png_bound bytes; a filter -1 .. 4; tEXt keys of 1 .. 79 bytes; "
		                                                "a display with a curve 0 .. 3, an exposure in [2^-40, 2^40], a white in [2^-10, 2^10], a dither 0 or 1)");
	const uint32_t n = (uint32_t)n64, rowBytes = 3u * (uint32_t)width, count = rowBytes * (uint32_t)height, at = (uint32_t)headBytes - 10u;
	const uint32_t segs = (n + CRX_SEG - 1u) / CRX_SEG, words = (n + 3u) / 4u, imgWords = (count + 3u) / 4u;
	const size_t bound = (size_t)pngBound(n64, headBytes);
	ZipGeom G;          /* one chunk of n bytes */
	memset(&G, 0, sizeof(G));
	G.nch = 1u; G.width = n; G.rowCount = 1u; G.lpc = 1u; G.nchunks = 1u; G.fullBytes = n; G.rowBytes = n; G.segsPerChunk = segs; G.pitch = words;

	HIP_TRY(hipSetDevice(c->device));
	int rc;
	if ((rc = c->dImg.grow(c->stream, imgWords))) return rc;
	if ((rc = c->dTypes.grow(c->stream, (size_t)height))) return rc;
	if ((rc = c->dT.grow(c->stream, words))) return rc;
	if ((rc = c->dSegOut.grow(c->stream, (size_t)segs * (CRX_SEG_OUT / 4u)))) return rc;
	if ((rc = c->dMeta.grow(c->stream, 7u * (size_t)segs + 4u))) return rc;
	if ((rc = c->dOut.grow(c->stream, bound))) return rc;
	if ((rc = growPinned(c, bound))) return rc;
	uint32_t *const segMeta = c->dMeta.p, *const segOff = segMeta + 4u * (size_t)segs, *const crcMeta = segOff + segs, *const info = crcMeta + 2u * (size_t)segs;
	const uint8_t *const img = (const uint8_t *)c->dImg.p;

	memcpy(c->pinned, head.data(), head.size());
	HIP_TRY(hipMemcpyAsync(c->dOut.p, c->pinned, head.size(), hipMemcpyHostToDevice, c->stream));
	if ((rc = c->pngWatch.start(c->stream))) return rc;
	const dim3 convertGrid((imgWords + 255u) / 256u);
	if (!display || displayIdentity(*display)) hipLaunchKernelGGL(k_png_convert, convertGrid, dim3(256), 0, c->stream, dev_fb, count, c->dImg.p);
	else {
		const PngDisplay d = {display->exposure, display->white * display->white, pngHable(2.0f * display->white), display->dither};
		const uint32_t w = (uint32_t)width;
		switch (display->curve) {
		case CRX_CURVE_CLAMP: hipLaunchKernelGGL(k_png_convert_display<CRX_CURVE_CLAMP>, convertGrid, dim3(256), 0, c->stream, dev_fb, count, w, d, c->dImg.p); break;
		case CRX_CURVE_REINHARD: hipLaunchKernelGGL(k_png_convert_display<CRX_CURVE_REINHARD>, convertGrid, dim3(256), 0, c->stream, dev_fb, count, w, d, c->dImg.p); break;
		case CRX_CURVE_ACES: hipLaunchKernelGGL(k_png_convert_display<CRX_CURVE_ACES>, convertGrid, dim3(256), 0, c->stream, dev_fb, count, w, d, c->dImg.p); break;
		default: hipLaunchKernelGGL(k_png_convert_display<CRX_CURVE_HABLE>, convertGrid, dim3(256), 0, c->stream, dev_fb, count, w, d, c->dImg.p); break;
		}
	}
	HIP_TRY(hipGetLastError());
	if ((rc = c->pngWatch.mark(c->stream))) return rc;
	hipLaunchKernelGGL(k_png_choose, dim3(((uint32_t)height + 3u) / 4u), dim3(256), 0, c->stream, img, rowBytes, (uint32_t)height, filter, c->dTypes.p);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_png_filter, dim3((words + 255u) / 256u), dim3(256), 0, c->stream, img, c->dTypes.p, rowBytes, n, c->dT.p);
	HIP_TRY(hipGetLastError());
	if ((rc = c->pngWatch.mark(c->stream))) return rc;
	if (c->codes == CRX_CODES_DYNAMIC) hipLaunchKernelGGL(k_zip_deflate_dynamic, dim3(segs), dim3(64), 0, c->stream, G, c->dT.p, c->dSegOut.p, segMeta);
	else hipLaunchKernelGGL(k_zip_deflate, dim3(segs), dim3(64), 0, c->stream, G, c->dT.p, c->dSegOut.p, segMeta);
	HIP_TRY(hipGetLastError());
	if ((rc = c->pngWatch.mark(c->stream))) return rc;
	hipLaunchKernelGGL(k_png_crc, dim3(segs), dim3(64), 0, c->stream, (const uint8_t *)c->dSegOut.p, CRX_SEG_OUT, segMeta, (uint64_t)0, crcMeta);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_png_scan, dim3(1), dim3(256), 0, c->stream, segMeta, crcMeta, segs, n, segOff, info);
	HIP_TRY(hipGetLastError());
	if ((rc = c->pngWatch.mark(c->stream))) return rc;
	hipLaunchKernelGGL(k_png_emit, dim3(segs), dim3(256), 0, c->stream, c->dSegOut.p, segMeta, segOff, info, c->dOut.p, at);
	HIP_TRY(hipGetLastError());
	if ((rc = c->pngWatch.mark(c->stream))) return rc;
	c->pngWatch.stop();

	/* the size first: it says how many bytes to fetch */
	uint32_t *const got = (uint32_t *)c->pinned;
	HIP_TRY(hipMemcpyAsync(got, info, 4u * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint64_t total = headBytes + got[0] + CRX_PNG_FIXED_TAIL;
	if (total > bound) return fail(CRH_ERR_HIP, "crx_png_pack: the device reported an impossible size");
	HIP_TRY(hipMemcpyAsync(c->pinned, c->dOut.p, total, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	memcpy(host_out, c->pinned, total);
	*total_bytes = total;
	return CRH_OK;
}
}  // namespace

extern "C" {

int crx_png_pack(crx_ctx *c, const float *dev_fb, int width, int height, int filter, const crx_png_text *text, uint32_t text_count, void *host_out, uint64_t capacity,
                 uint64_t *total_bytes) {
	return pngPack("crx_png_pack", c, dev_fb, width, height, nullptr, filter, text, text_count, host_out, capacity, total_bytes);
}

void crx_display_default(crx_display *d) {
	if (!d) return;
	d->exposure = 1.0f; d->curve = CRX_CURVE_CLAMP; d->white = 4.0f; d->dither = 0;
}

int crx_png_pack_display(crx_ctx *c, const float *dev_fb, int width, int height, const crx_display *display, int filter, const crx_png_text *text, uint32_t text_count,
                         void *host_out, uint64_t capacity, uint64_t *total_bytes) {
	return pngPack("crx_png_pack_display", c, dev_fb, width, height, display, filter, text, text_count, host_out, capacity, total_bytes);
}

int crx_auto_exposure(crx_ctx *c, const float *dev_fb, int width, int height, uint32_t permille, float target, float *exposure, float *key, uint64_t *counted) {
	uint64_t n = 0, headBytes = 0;
	if (!c || !dev_fb || !exposure || !key || !counted || !pngLayout(width, height, nullptr, 0u, &n, &headBytes, nullptr) || permille < 1u || permille > 1000u ||
	    !(target > 0.0f) || !(target < __builtin_inff()))
		return fail(CRH_ERR_INVALID, "crx_auto_exposure: bad argument (a context, a frame crx_png_pack takes, outputs; permille 1 .. 1000; a finite target > 0)");
	const uint32_t pixels = (uint32_t)width * (uint32_t)height;
	/* a workgroup a thousand pixels — four a lane — up to four workgroups a CU of the largest part: from one workgroup for 1 x 1 to a grid-stride pass */
	const uint32_t blocks = zipMin((pixels + 1023u) / 1024u, 1024u);
	HIP_TRY(hipSetDevice(c->device));
	int rc;
	if ((rc = c->dHist.grow(c->stream, CRX_HIST_BINS + 4u))) return rc;
	if ((rc = growPinned(c, 4u * sizeof(uint32_t)))) return rc;
	uint32_t *const result = c->dHist.p + CRX_HIST_BINS;
	HIP_TRY(hipMemsetAsync(c->dHist.p, 0, CRX_HIST_BINS * sizeof(uint32_t), c->stream));
	if ((rc = c->autoWatch.start(c->stream))) return rc;
	hipLaunchKernelGGL(k_png_histogram, dim3(blocks), dim3(256), 0, c->stream, dev_fb, pixels, c->dHist.p);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_png_pick, dim3(1), dim3(256), 0, c->stream, (const uint32_t *)c->dHist.p, permille, target, result);
	HIP_TRY(hipGetLastError());
	if ((rc = c->autoWatch.mark(c->stream))) return rc;
	c->autoWatch.stop();
	uint32_t *const got = (uint32_t *)c->pinned;
	HIP_TRY(hipMemcpyAsync(got, result, 4u * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	memcpy(exposure, &got[0], sizeof(float));
	memcpy(key, &got[1], sizeof(float));
	*counted = got[2];
	return CRH_OK;
}

int crx_auto_exposure_time_ms(crx_ctx *c, float *ms) {
	if (!c || !ms) return fail(CRH_ERR_INVALID, "crx_auto_exposure_time_ms: NULL argument");
	HIP_TRY(hipSetDevice(c->device));
	const int rc = c->autoWatch.read();
	if (rc) return rc;
	*ms = c->autoWatch.sum;
	return CRH_OK;
}

void crx_despeckle_default(crx_despeckle_params *p) {
	if (!p) return;
	p->radius = 2; p->rank = 4; p->factor = 4.0f; p->floor = 0x1p-6f;
}

int crx_despeckle(crx_ctx *c, const crx_despeckle_params *params, const float *dev_guide, int width, int height, float *const *dev_frames, uint32_t frame_count,
                  crx_despeckle_stats *stats) {
	crx_despeckle_params p;
	crx_despeckle_default(&p);
	if (params) p = *params;
	uint64_t n = 0, headBytes = 0;
	bool ok = c && dev_guide && pngLayout(width, height, nullptr, 0u, &n, &headBytes, nullptr) && (p.radius == 1 || p.radius == 2) && p.rank >= 1 &&
	          p.rank <= (2 * p.radius + 1) * (2 * p.radius + 1) - 1 && p.factor >= 1.0f && p.factor <= CRX_DESPECKLE_FACTOR_MAX && p.floor >= 0.0f &&
	          p.floor <= CRX_DESPECKLE_FLOOR_MAX && frame_count <= CRX_DESPECKLE_MAX_FRAMES && (dev_frames || !frame_count);          /* (a NaN fails every comparison) */
	for (uint32_t i = 0; ok && i < frame_count; ++i) ok = dev_frames[i] != nullptr;
	if (!ok)
		return fail(CRH_ERR_INVALID, "crx_despeckle: bad argument (a context, a guide frame crx_png_pack takes; radius 1 or 2, rank 1 .. (2 radius + 1)^2 - 1, a factor in "
		                             "[1, 2^20], a floor in [0, 2^20]; at most 8 frames, none NULL)");
	const uint32_t pixels = (uint32_t)width * (uint32_t)height, planeWords = (pixels + 3u) / 4u * 4u;
	const uint32_t tilesX = ((uint32_t)width + DS_TILE_W - 1u) / DS_TILE_W, tilesY = ((uint32_t)height + DS_TILE_H - 1u) / DS_TILE_H;          /* (tilesX * tilesY <= pixels < 2^30) */
	const DsParams P = {p.factor, p.floor, (uint32_t)p.rank};
	HIP_TRY(hipSetDevice(c->device));
	int rc;
	c->scaleWidth = c->scaleHeight = 0;
	if ((rc = c->dScale.grow(c->stream, (size_t)planeWords + 4u))) return rc;
	if ((rc = growPinned(c, 8u * sizeof(uint32_t)))) return rc;
	float *const plane = (float *)c->dScale.p;
	uint32_t *const devStats = c->dScale.p + planeWords, *const init = (uint32_t *)c->pinned, *const got = init + 4;
	init[0] = 0u; init[1] = 0u; init[2] = 0u; init[3] = 0x3f800000u;          /* no clamped pixel: max_clamped 0, min_scale 1 */
	HIP_TRY(hipMemcpyAsync(devStats, init, 4u * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	if ((rc = c->despeckleWatch.start(c->stream))) return rc;
	if (p.radius == 1) hipLaunchKernelGGL(k_despeckle_measure<1>, dim3(tilesX * tilesY), dim3(256), 0, c->stream, dev_guide, (uint32_t)width, (uint32_t)height, tilesX, P, plane, devStats);
	else hipLaunchKernelGGL(k_despeckle_measure<2>, dim3(tilesX * tilesY), dim3(256), 0, c->stream, dev_guide, (uint32_t)width, (uint32_t)height, tilesX, P, plane, devStats);
	HIP_TRY(hipGetLastError());
	if ((rc = c->despeckleWatch.mark(c->stream))) return rc;
	for (uint32_t i = 0; i < frame_count; ++i) {          /* in stream order behind the measure launch: the guide may be among the frames */
		hipLaunchKernelGGL(k_despeckle_apply, dim3((pixels + 1023u) / 1024u), dim3(256), 0, c->stream, (const float *)plane, pixels, dev_frames[i]);
		HIP_TRY(hipGetLastError());
	}
	if ((rc = c->despeckleWatch.mark(c->stream))) return rc;
	c->despeckleWatch.stop();
	HIP_TRY(hipMemcpyAsync(got, devStats, 4u * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	c->scaleWidth = width; c->scaleHeight = height;
	if (stats) {
		stats->clamped = got[0]; stats->bad = got[1];
		memcpy(&stats->max_clamped, &got[2], sizeof(float));
		memcpy(&stats->min_scale, &got[3], sizeof(float));
	}
	return CRH_OK;
}

int crx_despeckle_scale(crx_ctx *c, float *host_scale) {
	if (!c || !host_scale || c->scaleWidth <= 0) return fail(CRH_ERR_INVALID, "crx_despeckle_scale: bad argument (a context with a complete crx_despeckle behind it, an output)");
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipMemcpyAsync(host_scale, c->dScale.p, (size_t)c->scaleWidth * (size_t)c->scaleHeight * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return CRH_OK;
}

int crx_despeckle_time_ms(crx_ctx *c, float ms[2]) {
	if (!c || !ms) return fail(CRH_ERR_INVALID, "crx_despeckle_time_ms: NULL argument");
	HIP_TRY(hipSetDevice(c->device));
	const int rc = c->despeckleWatch.read();
	if (rc) return rc;
	for (int i = 0; i < 2; ++i) ms[i] = i < c->despeckleWatch.laps ? c->despeckleWatch.ms[i] : 0.0f;
	return CRH_OK;
}

int crx_png_phases_ms(crx_ctx *c, float phases_ms[CRX_PNG_PHASES]) {
	if (!c || !phases_ms) return fail(CRH_ERR_INVALID, "crx_png_phases_ms: NULL argument");
	HIP_TRY(hipSetDevice(c->device));
	const int rc = c->pngWatch.read();
	if (rc) return rc;
	for (int i = 0; i < CRX_PNG_PHASES; ++i) phases_ms[i] = i < c->pngWatch.laps ? c->pngWatch.ms[i] : 0.0f;
	return CRH_OK;
}

int crx_debug_crc32(crx_ctx *c, const void *host_bytes, uint64_t n, uint32_t piece_bytes, uint32_t *crc) {
	if (!c || !crc || !piece_bytes || (n && !host_bytes) || n >= (1ull << 32) || (n + piece_bytes - 1u) / piece_bytes >= (1ull << 28))
		return fail(CRH_ERR_INVALID, "crx_debug_crc32: bad argument (below 2^32 bytes in fewer than 2^28 pieces of at least one byte)");
	const uint32_t pieces = (uint32_t)((n + piece_bytes - 1u) / piece_bytes);
	HIP_TRY(hipSetDevice(c->device));
	int rc;
	if ((rc = c->dT.grow(c->stream, (size_t)(n + 3u) / 4u + 1u))) return rc;
	if ((rc = c->dMeta.grow(c->stream, 2u * (size_t)pieces + 4u))) return rc;
	uint32_t *const crcMeta = c->dMeta.p, *const info = crcMeta + 2u * (size_t)pieces;
	if (n) HIP_TRY(hipMemcpyAsync(c->dT.p, host_bytes, n, hipMemcpyHostToDevice, c->stream));
	if (pieces) {
		hipLaunchKernelGGL(k_png_crc, dim3(pieces), dim3(64), 0, c->stream, (const uint8_t *)c->dT.p, piece_bytes, (const uint32_t *)nullptr, n, crcMeta);
		HIP_TRY(hipGetLastError());
	}
	hipLaunchKernelGGL(k_png_scan, dim3(1), dim3(256), 0, c->stream, (const uint32_t *)nullptr, crcMeta, pieces, 0u, (uint32_t *)nullptr, info);
	HIP_TRY(hipGetLastError());
	uint32_t got[4];
	HIP_TRY(hipMemcpyAsync(got, info, sizeof(got), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	*crc = got[2];
	return CRH_OK;
}

}  // extern "C"
