/*
 * renderer_hip.c — drop-in replacement for the reference's src/renderer/renderer.c.
 *
 * It exports exactly the three symbols the rest of c-ray links against (src/renderer/renderer.h:101-107):
 *     struct renderer *newRenderer(void);
 *     struct texture  *renderFrame(struct renderer *r);     <- THE boundary (called from src/c-ray.c:280)
 *     void             destroyRenderer(struct renderer *r);
 * and leaves struct renderer / state / prefs / renderThreadState untouched, so src/c-ray.c, the JSON loader,
 * tile.c, ui.c (SDL2 preview) and the PNG/BMP encoders keep working unmodified.
 *
 * What changes is who consumes the tile queue: instead of N pthread workers running the pixel x pass loop
 * (renderer.c:258-327) there is ONE host thread per GPU. The scene is flattened once (flatten.c) by the main thread WHILE the GPU threads
 * create their contexts, allocate the per-wave buffers and load the kernels' code objects (crh_context_prepare) and a helper thread
 * creates the RCCL communicators (crh_frames_prepare): none of that is left inside the frame's timed part. Each GPU thread then uploads the
 * scene and renders ITS share of the frame — one GPU: the whole frame as one region; several: every G-th 4-row strip — in dispatches of
 * as many passes as take about a second (the persistent kernel balances the work units inside a dispatch itself; a frame is cut only along the
 * pass axis, so that the preview window, the abort and the pause key get a turn). Between two dispatches the thread converts its share to
 * 8-bit sRGB ON THE DEVICE (crh_framebuffer_to_srgb8: colorToSRGB + setPixel's truncation, bit for bit) into `output`, which the main
 * thread keeps drawing (renderer.c:294-300 wrote it per sample). At the end the GPUs' strips are gathered onto GPU 0 with RCCL over xGMI
 * (crh_frames_gather: 1/G of the frame per link; CRH_FRAMES=reduce selects the one-ncclReduce form), the 8-bit frame and the float buffer
 * come back with one download each.
 *
 * --iterative (renderThreadInteractive, renderer.c:184-250): passes 1 .. sampleCount-1 with the Halton sampler, the frame
 * shown while it converges. Here the main thread drives every GPU (every G-th 4-row strip belongs to one GPU for the whole frame, so each
 * pixel's running mean stays on one GPU) in dispatches of as many passes as take about 16 ms, converts to 8-bit on the device after each
 * and redraws; the float buffer is gathered once, at the end. The result is the reference's single-thread result: with several threads the
 * reference itself races on state.finishedPasses and is not reproducible.
 *
 * A GPU that fails — at set-up or in the middle of the frame — does not end the program: its strips (a pure function of (g, G): share.h) are dealt to the
 * GPUs that finished and rendered there from pass 0, the way the reference's cluster master re-issues the tiles of a worker it lost (src/datatypes/tile.c:31-42);
 * that frame is assembled on the host (the survivors' buffers merged: a pixel has one owner, everybody else holds 0.0f there). Only when NO GPU is left
 * does renderFrame() end with logr(error, ...).
 *
 * Environment: CRAY_HIP_DEVICES=<n> caps the number of GPUs used; CRH_DROPIN_PASSES=<n> (dev / tests) fixes the passes per dispatch; CRH_DUMP_F32=<path> dumps the float buffer; CRH_DUMP_STATS=<path>
 * writes where the frame's time went; CRH_FRAMES=reduce: see above. CRAY_HIP_AOV=<n> (user-facing, like CRAY_HIP_WALK): after the frame, GPU 0 renders the guide buffers
 * a denoiser or a compositor asks for — albedo, normal, depth of every camera ray's first hit, n passes of them (crh_render_aov) — and writes them beside the frame
 * through the reference's own encoders (writeAovs below); CRH_DUMP_AOV_F32=<path> dumps their floats. CRAY_HIP_DENOISE=<iterations> (user-facing): GPU 0 renders the guides,
 * filters the frame with them (crh_denoise) into a buffer of its own and writes <imgFileName>_denoised beside the frame (writeDenoised below); CRH_DUMP_DENOISED_F32=<path>
 * dumps its floats. The frame, its image and the returned texture are untouched. CRAY_HIP_DENOISE_VARIANCE=1 beside it: the filter is crh_denoise_variance — every GPU
 * thread ends a dispatch exactly at pass sampleCount / 2 and keeps a copy of its frame buffer there (crh_framebuffer_copy), the copies are assembled on GPU 0 like
 * the frame; consecutive pass ranges compose bit for bit, so the frame is the one of a run without the variable.
 * CRAY_HIP_DESPECKLE=<factor> beside CRAY_HIP_DENOISE (user-facing; CRAY_HIP_DESPECKLE_RANK, _RADIUS, _FLOOR beside it): the denoiser reads a despeckled copy of the
 * frame — and of the half-sample frame, under the same plane — in which fireflies are scaled down to a rank of their neighbourhood (crx_despeckle of
 * libcray_hip_exr.so; despeckledCopies below). The frame, its image, the returned texture, R G B of the layers file and the GPU PNG stay as they are. Without
 * CRAY_HIP_DENOISE: a warning and no effect. A bad value: a warning and the plain denoise. Unset: nothing of it runs.
 * CRAY_HIP_ADAPTIVE=<threshold> (user-facing; CRAY_HIP_ADAPTIVE_MIN=<m>, default 16): adaptive sampling at tile granularity — every GPU thread hands its rectangles
 * (one GPU: the scene's tileWidth x tileHeight grid; several: its strips cut every tileWidth columns) to crh_render_adaptive, which gives every rectangle m passes
 * and doubles that until its error is at most the threshold or sampleCount is reached; a sampleCount that is not m 2^r: a warning and the uniform frame.
 * CRAY_HIP_ADAPTIVE_CELL=<c> (user-facing, beside CRAY_HIP_ADAPTIVE; CRAY_HIP_ADAPTIVE_DILATE=0|1, default 1): the same rectangles, decided per c x c cell inside each
 * (crh_render_adaptive_cells); the report line counts cells by pass count. A value that is no integer in 1 .. 1024, or a rectangle of more than 1024 cells, warns
 * and decides per rectangle.
 * CRAY_HIP_EXR=1 (user-facing): one multi-layer OpenEXR file <imgFileName>_layers beside the frame — the frame's floats, and whatever CRAY_HIP_AOV and CRAY_HIP_DENOISE
 * produced, unscaled: the buffers stay on GPU 0 until writeLayers below has packed them (crh_pack_scanlines) —; CRAY_HIP_IDS=<n> beside it: GPU 0 also renders n passes
 * of the instance and material ID buffers (crh_render_ids), which go into the file as Cryptomatte layers named after the scene's meshes. The frame, its image and the
 * other side files are those of a run without the two. CRAY_HIP_EXR_COMPRESSION=zip|zips beside it: the file is ZIP / ZIPS compressed, deflated on the device.
 * CRAY_HIP_EXR_HALF=1 beside it: the colour layers (R G B, albedo.*, normal.*, denoised.*) are 16-bit HALF channels, Z, A and the Cryptomatte channels stay FLOAT
 * (crx_pack of libcray_hip_exr.so, for every compression); values above 65504 become infinity in them. Anything else or unset: all FLOAT.
 * CRAY_HIP_EXR_CODES=dynamic beside CRAY_HIP_EXR_COMPRESSION: every segment of a chunk is deflated with the cheaper of the fixed Huffman codes and a dynamic code
 * built on the device (crx_set_codes): the same pixels in a smaller file. Anything else or unset: the fixed codes.
 * CRAY_HIP_PNG=1 (user-facing): the frame on GPU 0 also as <imgFileName>_gpu_<count>.png, encoded on the device (writeGpuPng below: crx_png_pack), with tEXt chunks for the
 * sample and bounce counts, next to the frame's own file, which writeImage writes as ever. Dynamic codes unless CRAY_HIP_EXR_CODES=fixed. Unset: nothing of it runs.
 * CRAY_HIP_PNG_EXPOSURE=<float>|auto, CRAY_HIP_PNG_TONEMAP=clamp|reinhard|aces|hable, CRAY_HIP_PNG_WHITE=<float>, CRAY_HIP_PNG_DITHER=1 beside it: the display
 * transform of that file (crx_png_pack_display; auto: crx_auto_exposure takes the median luminance to 0.18), named in a third tEXt chunk "C-ray Display" and in the log.
 * None set: the file of CRAY_HIP_PNG=1 alone, byte for byte. A bad value: a warning, and the file without a transform.
 * No GPU => logr(error, ...) (which exits, src/utils/logging.c:69-73): there is no CPU fallback in this file.
 */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <stdbool.h>
#include <pthread.h>
#include <errno.h>
#include <time.h>

#include "includes.h"
#include "datatypes/image/imagefile.h"
#include "renderer/renderer.h"
#include "datatypes/image/texture.h"
#include "datatypes/color.h"
#include "datatypes/scene.h"
#include "datatypes/mesh.h"
#include "datatypes/tile.h"
#include "datatypes/vertexbuffer.h"
#include "utils/ui.h"
#include "utils/logging.h"
#include "utils/timer.h"
#include "utils/platform/thread.h"
#include "utils/platform/mutex.h"
#include "utils/args.h"
#include "utils/encoders/encoder.h"

#include "cray_hip.h"
#include "cray_hip_exr.h"
#include "flatten.h"
#include "exr_write.h"
#include "share.h"

#define MAX_GPUS 16

/* what the main thread and the GPU threads tell each other: "the scene is flattened" (main -> GPUs), "a GPU thread has finished" (GPUs -> main) */
struct frameSync {
	pthread_mutex_t mu;
	pthread_cond_t cv;
	int sceneReady;          /* 1: flattened (and, for several GPUs, compiled), -1: the flattener / the layout compile failed */
	const crh_compiled_scene *compiled;          /* several GPUs: the device layout, derived ONCE by the main thread (round 5: every GPU thread used to derive it for itself); NULL: one GPU,
	                                              * whose crh_scene_upload compiles with its texel copy beside it */
	int finished;
	int launched;            /* GPU threads whose first dispatch is on its device (or that ended before one): the flattened scene has been read for the last time */
};

struct gpuWorker {
	struct renderer *r;
	struct renderThreadState *state;
	const crh_scene_desc *scene;
	struct frameSync *sync;
	struct texture *output;
	struct timeval frameStart;   /* renderFrame() entry */
	crh_ctx *ctx;
	float *fb;
	float *half;          /* CRAY_HIP_DENOISE_VARIANCE: the frame buffer as it was after the first sampleCount / 2 passes; CRAY_HIP_ADAPTIVE: every rectangle's after the first half of ITS passes */
	crh_tile *adaptTiles;     /* CRAY_HIP_ADAPTIVE: this GPU's rectangles and the pass count each stopped at */
	int32_t *adaptPasses;
	uint32_t adaptCount;
	uint32_t adaptUnits;      /* entries of adaptPasses: the rectangles, or with CRAY_HIP_ADAPTIVE_CELL their cells */
	int adaptCell;            /* the cell size the frame was decided at; 0: per rectangle */
	int device;
	int failed;
	char error[256];      /* crh_last_error() is per thread: the failing dispatch thread keeps its message here */
	uint64_t rays;
	int announced;                        /* sync->launched counts this thread */
	long contextUs, uploadUs, renderUs;   /* context + buffers + code objects (beside the flattener); scene upload + framebuffer; dispatch loop (first launch to last sync) */
	long readyUs;             /* renderFrame() entry -> this GPU ready to dispatch */
	double kernelMs;          /* GPU time of the dispatches (HIP events around the kernels) */
	long launchUs;            /* host time inside crh_render_tiles (work list, copies, launch) */
	int dispatches;
};

/* A dispatch keeps the whole GPU busy from its first work unit to its last (no drain in between), so a frame is cut only along the pass
 * axis, and only when it is long: the first dispatch takes as many passes as make FIRST_DISPATCH_PATHS paths (the bench frame: all 256),
 * the following ones as many as took about DISPATCH_TARGET_MS at the measured rate — the preview, the abort and the pause key wait no
 * longer than that. */
#define FIRST_DISPATCH_PATHS (256ull << 20)
#define DISPATCH_TARGET_MS 1000.0

/* The share of GPU g of G: G == 1 -> the whole frame; G > 1 -> every G-th 4-row strip
 * (static shares must be balanced, and dealing out the tile list is not: DESIGN.md section 6). Returns the tile count. */
static uint32_t gpuShare(const struct renderer *r, int g, int G, crh_tile **out) {
	const int W = (int)r->prefs.imageWidth, H = (int)r->prefs.imageHeight;
	if (G == 1) {
		/* the whole frame as one region: inside a dispatch the library hands out the pixel blocks bottom-up, row by row. The order of the
		 * reference's tile list (tile.c:119-241) is a preview preference, not part of the result — and measured on one GPU it costs 2 %
		 * (fromMiddle) to 10 % (topToBottom: the expensive bottom of a frame ends up in the small blocks of the dispatch's tail) */
		crh_tile *t = calloc(1, sizeof(*t));
		t[0] = (crh_tile){0, 0, W, H};
		*out = t;
		return 1;
	}
	crh_tile *t = calloc((size_t)crh_strip_share_max(H, G), sizeof(*t));
	*out = t;
	return crh_strip_share(W, H, g, G, t);
}

/* renderer.c:294-300 for this GPU's share: colorToSRGB + setPixel's truncation on the device, then the rows of ITS strips into `output` (texture.c:18-22
 * layout, the float buffer's) — one strided copy of 1 / G of the 8-bit frame (crh_framebuffer_strips_to_srgb8). */
static int refreshOutput(crh_ctx *ctx, const float *fb, int W, int H, struct texture *output, int g, int G) {
	return crh_framebuffer_strips_to_srgb8(ctx, fb, W, H, CRH_STRIP_ROWS, g, G, output->data.byte_p);
}

/* A throw-away dispatch ends a GPU's set-up: a few pixels, one pass, into the (still empty) framebuffer, which is cleared again. Measured in round 3
 * (CRH_TRACE_SYNC, profiles/r03l_probe_dropin.log): the first kernel of a process that does real work starts 5-24 ms after its launch — whatever was copied,
 * synchronized, launched empty or waited for before it — and the second does not; that first one should not be the frame. CRH_DROPIN_NO_WARM=1 leaves it out. */
static void warmUp(crh_ctx *ctx, float *fb, const crh_render_params *p, int device) {
	if (getenv("CRH_DROPIN_NO_WARM")) return;
	crh_render_params wp = *p;
	wp.x0 = 0; wp.y0 = 0; wp.x1 = p->image_width < 64 ? p->image_width : 64; wp.y1 = p->image_height < 16 ? p->image_height : 16;
	wp.first_pass = 0; wp.pass_count = 1;
	if (crh_render_region(ctx, &wp, fb) != CRH_OK || crh_synchronize(ctx) != CRH_OK || crh_framebuffer_clear(ctx, fb, p->image_width, p->image_height) != CRH_OK ||
		crh_counters_reset(ctx) != CRH_OK || crh_synchronize(ctx) != CRH_OK)
		logr(warning, "GPU %d: warm-up dispatch: %s\n", device, crh_last_error());
}

/* ---- the process's render contexts ------------------------------------------------------------------------------------------------------------
 * A context ready to dispatch — stream, counters, code objects, 600 MB of per-wave buffers — takes 13-30 ms to make (round 4, CRH_TRACE_UPLOAD: 8 ms until it
 * exists, 5-21 ms until crh_context_prepare returns) and 5 ms to take down, and none of it depends on the scene. They are therefore made — one thread per
 * device — from newRenderer() on, while the program spends hundreds of milliseconds parsing JSON and OBJ files, and a frame's contexts go back to this pool instead
 * of being destroyed inside renderFrame(); destroyRenderer() ends them. A dispatch thread whose device has no context yet (the maker failed, more GPUs than
 * MAX_GPUS makers) makes it beside the flattener, as before. CRH_DROPIN_NO_PREFETCH=1: every context is made inside renderFrame();
 * CRH_DROPIN_PREFETCH_GPUS=n: makers for the first n devices only (a scene file that asks for fewer GPUs than the node has). */
static struct {
	pthread_mutex_t mu, joinMu;          /* joinMu: one thread joins the master, the others wait until it has (a maker that is not started yet would be missed) */
	crh_ctx *ctx[MAX_GPUS];
	pthread_t master, maker[MAX_GPUS];
	int masterLive, makerLive[MAX_GPUS];
} g_pool = {.mu = PTHREAD_MUTEX_INITIALIZER, .joinMu = PTHREAD_MUTEX_INITIALIZER};

/* CRAY_HIP_WALK=wide4: the frame renderer walks the 4-ary copy of the BVHs (CRH_OPT_WALK; venus.json +10 %, statues / soups +3 %, frames not bit-identical to the
 * reference's where two hits nearly tie: an opt-in). Anything else: the reference's walk */
static int frameWalk(void) {
	const char *e = getenv("CRAY_HIP_WALK");
	return e && !strcmp(e, "wide4") ? CRH_WALK_WIDE4 : CRH_WALK_BINARY;
}

static crh_ctx *makeContext(int device) {
	crh_ctx *c = NULL;
	if (crh_abi_version() != CRH_ABI_VERSION) {          /* this file is built with the header of the library it expects */
		logr(warning, "c-ray-hip: libcray_hip has ABI version %i, this program was built for %i\n", crh_abi_version(), CRH_ABI_VERSION);
		return NULL;
	}
	/* counter level 1: this host reports rays only (the detailed counters cost ~20 % of the kernel's time) */
	if (crh_context_create(device, NULL, &c) != CRH_OK) return NULL;
	if (crh_set_option(c, CRH_OPT_COUNTER_LEVEL, 1) != CRH_OK || crh_set_option(c, CRH_OPT_WALK, frameWalk()) != CRH_OK ||
		(!getenv("CRH_DROPIN_NO_PREPARE") && crh_context_prepare(c) != CRH_OK)) {
		crh_context_destroy(c);
		return NULL;
	}
	return c;
}

static void *makerThread(void *arg) {
	const int device = (int)(intptr_t)arg;
	crh_ctx *c = makeContext(device);
	pthread_mutex_lock(&g_pool.mu);
	g_pool.ctx[device] = c;
	pthread_mutex_unlock(&g_pool.mu);
	return NULL;
}

/* counts the devices (the first HIP call of the process: not on the thread that is about to parse the scene) and starts one maker per device the frame will use:
 * renderFrame() renders on every visible GPU, CRAY_HIP_DEVICES=n on the first n */
static void *masterThread(void *arg) {
	(void)arg;
	int n = crh_device_count();
	if (n > MAX_GPUS) n = MAX_GPUS;
	const char *cap = getenv("CRAY_HIP_DEVICES");          /* the same cap renderFrame() applies: no context on a GPU the frame will not use */
	if (cap && atoi(cap) > 0 && atoi(cap) < n) n = atoi(cap);
	if (getenv("CRH_DROPIN_PREFETCH_GPUS") && atoi(getenv("CRH_DROPIN_PREFETCH_GPUS")) < n) n = atoi(getenv("CRH_DROPIN_PREFETCH_GPUS"));
	for (int g = 0; g < n; ++g) {
		pthread_mutex_lock(&g_pool.mu);
		if (!g_pool.makerLive[g] && !g_pool.ctx[g] && pthread_create(&g_pool.maker[g], NULL, makerThread, (void *)(intptr_t)g) == 0) g_pool.makerLive[g] = 1;
		pthread_mutex_unlock(&g_pool.mu);
	}
	return NULL;
}

static void poolJoin(int device);
/* (a stated limit: this handler covers the context MAKERS. A logr(error) -> exit() from inside renderFrame / renderInteractive while the frame's GPU threads have
 * dispatches in flight is not waited for here — those threads block in crh_synchronize for the length of a frame, and exit() would hang as long; the reference's own worker
 * threads are not joined on that path either: renderer.c:96-117 —, and a maker that hangs inside hipMalloc holds exit() up with it.) */
/* the process never exits with HIP calls in flight (logr(error) exit()s on a scene the parser rejects, while the makers may be inside hipMalloc or a code-object
 * load — ROCm's teardown is known to crash then): exit() waits for the makers here; the contexts themselves are left to the process's end */
static void poolAtExit(void) {
	for (int g = 0; g < MAX_GPUS; ++g) poolJoin(g);
}

static void poolPrefetch(void) {
	if (getenv("CRH_DROPIN_NO_PREFETCH")) return;
	static int hooked;
	if (!hooked) { hooked = 1; atexit(poolAtExit); }
	pthread_mutex_lock(&g_pool.mu);
	if (!g_pool.masterLive && pthread_create(&g_pool.master, NULL, masterThread, NULL) == 0) g_pool.masterLive = 1;
	pthread_mutex_unlock(&g_pool.mu);
}

static void poolJoin(int device) {
	pthread_mutex_lock(&g_pool.joinMu);
	pthread_mutex_lock(&g_pool.mu);
	const int master = g_pool.masterLive;
	g_pool.masterLive = 0;
	pthread_mutex_unlock(&g_pool.mu);
	if (master) pthread_join(g_pool.master, NULL);          /* (it only counts and starts) */
	pthread_mutex_unlock(&g_pool.joinMu);
	pthread_mutex_lock(&g_pool.mu);
	const int live = g_pool.makerLive[device];
	g_pool.makerLive[device] = 0;
	pthread_mutex_unlock(&g_pool.mu);
	if (live) pthread_join(g_pool.maker[device], NULL);
}

/* a context for `device`, ready to dispatch: the pool's, or a new one (NULL: crh_last_error() of the calling thread says why) */
static crh_ctx *poolAcquire(int device) {
	poolJoin(device);
	pthread_mutex_lock(&g_pool.mu);
	crh_ctx *c = g_pool.ctx[device];
	g_pool.ctx[device] = NULL;
	pthread_mutex_unlock(&g_pool.mu);
	return c ? c : makeContext(device);
}

static void poolRelease(int device, crh_ctx *c, int healthy) {
	if (!c) return;
	pthread_mutex_lock(&g_pool.mu);
	const int keep = healthy && !g_pool.ctx[device];
	if (keep) g_pool.ctx[device] = c;
	pthread_mutex_unlock(&g_pool.mu);
	if (!keep) crh_context_destroy(c);
}

static void poolDestroy(void) {
	for (int g = 0; g < MAX_GPUS; ++g) {
		poolJoin(g);
		pthread_mutex_lock(&g_pool.mu);
		crh_ctx *c = g_pool.ctx[g];
		g_pool.ctx[g] = NULL;
		pthread_mutex_unlock(&g_pool.mu);
		if (c) crh_context_destroy(c);
	}
}

/* CRAY_HIP_DENOISE=<iterations> with CRAY_HIP_DENOISE_VARIANCE=1: the pass at which every GPU thread copies its frame buffer, h = sampleCount / 2; 0: no copy
 * (the variable is unset, means nothing without CRAY_HIP_DENOISE, or the frame has fewer than two passes to split) */
static int varianceHalfPasses(const struct renderer *r) {
	const char *d = getenv("CRAY_HIP_DENOISE"), *v = getenv("CRAY_HIP_DENOISE_VARIANCE");
	if (!d || atoi(d) <= 0 || !v || atoi(v) <= 0 || r->prefs.sampleCount < 2) return 0;
	return r->prefs.sampleCount / 2;
}

/* CRAY_HIP_ADAPTIVE=<threshold> [CRAY_HIP_ADAPTIVE_MIN=<m>, default 16]: 1 and the two settings when the frame is rendered adaptively; 0 when the variable is unset
 * or the settings cannot be used (a threshold that is no number or negative, an m that is odd or below 2, a sampleCount that is not m 2^r) — the frame is
 * then rendered uniformly, as without the variable (renderFrame says so once) */
static int adaptiveSettings(const struct renderer *r, crh_adaptive_params *out) {
	const char *t = getenv("CRAY_HIP_ADAPTIVE"), *m = getenv("CRAY_HIP_ADAPTIVE_MIN");
	if (!t || !*t) return 0;
	crh_adaptive_params a;
	crh_adaptive_params_default(&a);
	char *end = NULL;
	a.threshold = strtof(t, &end);
	if (end == t || a.threshold != a.threshold || a.threshold < 0.0f) return 0;
	if (m && *m) a.min_passes = atoi(m);
	if (a.min_passes < 2 || (a.min_passes & 1)) return 0;
	long n = a.min_passes;
	while (n < r->prefs.sampleCount) n *= 2;
	if (n != r->prefs.sampleCount) return 0;
	if (out) *out = a;
	return 1;
}

/* CRAY_HIP_ADAPTIVE_CELL=<c> [CRAY_HIP_ADAPTIVE_DILATE=0|1, default 1] beside CRAY_HIP_ADAPTIVE: the decision is made per c x c cell inside every rectangle
 * (crh_render_adaptive_cells). 1 and the two settings; 0 when the variable is unset; -1 when its value is not an integer in 1 .. 1024 (renderFrame says so once,
 * and the frame is decided per rectangle). */
static int adaptiveCellSettings(int *cell, int *dilate) {
	const char *c = getenv("CRAY_HIP_ADAPTIVE_CELL"), *d = getenv("CRAY_HIP_ADAPTIVE_DILATE");
	if (!c || !*c) return 0;
	char *end = NULL;
	const long v = strtol(c, &end, 10);
	if (end == c || *end || v < 1 || v > 1024) return -1;
	if (cell) *cell = (int)v;
	if (dilate) *dilate = !(d && d[0] == '0' && !d[1]);
	return 1;
}

/* The rectangles crh_render_adaptive decides on, from a GPU's share: one GPU — the whole frame — gets the scene's tile grid (tile.c:66-117 without the ordering,
 * which is a preview preference), a GPU of several gets its strips cut every tileWidth columns. */
static uint32_t adaptiveRectangles(const struct renderer *r, const crh_tile *share, uint32_t n, int G, crh_tile **out) {
	const int tw = r->prefs.tileWidth >= 1 ? (int)r->prefs.tileWidth : 1, th = r->prefs.tileHeight >= 1 ? (int)r->prefs.tileHeight : 1;
	size_t count = 0;
	for (int pass = 0; pass < 2; ++pass) {          /* count, then fill */
		size_t k = 0;
		for (uint32_t i = 0; i < n; ++i) {
			const crh_tile s = share[i];
			const int stepY = G == 1 ? th : s.y1 - s.y0;
			for (int y = s.y0; y < s.y1; y += stepY)
				for (int x = s.x0; x < s.x1; x += tw, ++k)
					if (pass) (*out)[k] = (crh_tile){x, y, x + tw < s.x1 ? x + tw : s.x1, y + stepY < s.y1 ? y + stepY : s.y1};
		}
		if (!pass) { count = k; *out = calloc(count ? count : 1, sizeof(**out)); if (!*out) return 0; }
	}
	return (uint32_t)count;
}

static void announceLaunch(struct gpuWorker *w) {
	if (w->announced) return;
	w->announced = 1;
	pthread_mutex_lock(&w->sync->mu);
	w->sync->launched++;
	pthread_cond_broadcast(&w->sync->cv);
	pthread_mutex_unlock(&w->sync->mu);
}

static void gpuThreadDone(struct gpuWorker *w) {
	announceLaunch(w);
	w->state->currentTileNum = -1;
	w->state->threadComplete = true;
	pthread_mutex_lock(&w->sync->mu);
	w->sync->finished++;
	pthread_cond_broadcast(&w->sync->cv);
	pthread_mutex_unlock(&w->sync->mu);
}

static void *gpuThread(void *arg) {
	struct gpuWorker *w = threadUserData(arg);
	struct renderer *r = w->r;
	const int W = (int)r->prefs.imageWidth, H = (int)r->prefs.imageHeight;
	const int G = r->prefs.threadCount;
	crh_render_params p;
	memset(&p, 0, sizeof(p));
	p.image_width = W; p.image_height = H;
	p.max_passes = r->prefs.sampleCount;
	p.bounces = r->prefs.bounces;
	struct timeval phase;
	startTimer(&phase);

	/* beside the flattener: the context, the per-wave buffers, the code objects.
	 * counter level 1: this host reports rays only (the detailed counters cost ~20 % of the kernel's time) */
	w->ctx = poolAcquire(w->device);
	const long preparedUs = getUs(phase);
	/* (a pooled context has rendered before in this process: the frame's ray count starts at zero — ADVICE r05) */
	crh_adaptive_params adaptive;
	const int adapt = adaptiveSettings(r, &adaptive);
	const int halfAt = adapt ? 0 : varianceHalfPasses(r);          /* (an adaptive render keeps the half-sample frame itself) */
	int ok = w->ctx != NULL && crh_counters_reset(w->ctx) == CRH_OK && crh_framebuffer_alloc(w->ctx, W, H, &w->fb) == CRH_OK
		&& ((!halfAt && !adapt) || crh_framebuffer_alloc(w->ctx, W, H, &w->half) == CRH_OK);
	if (getenv("CRH_TRACE_UPLOAD"))
		fprintf(stderr, "gpuThread trace: GPU %d has its context (pool, or created + code objects + per-wave buffers) after %.1f ms, its framebuffer after %.1f ms\n",
				w->device, preparedUs / 1e3, getUs(phase) / 1e3);
	if (!ok) snprintf(w->error, sizeof(w->error), "%s", crh_last_error());
	w->contextUs = getUs(phase);
	pthread_mutex_lock(&w->sync->mu);
	while (!w->sync->sceneReady) pthread_cond_wait(&w->sync->cv, &w->sync->mu);
	const int sceneOk = w->sync->sceneReady > 0;
	pthread_mutex_unlock(&w->sync->mu);
	startTimer(&phase);
	if (ok && sceneOk && ((w->sync->compiled ? crh_scene_upload_compiled(w->ctx, w->sync->compiled) : crh_scene_upload(w->ctx, w->scene)) != CRH_OK ||
		crh_synchronize(w->ctx) != CRH_OK)) {           /* the scene copies are asynchronous: they belong to the setup, not to the first dispatch */
		snprintf(w->error, sizeof(w->error), "%s", crh_last_error());
		ok = 0;
	}
	if (!ok || !sceneOk) {
		if (!ok) logr(warning, "GPU %d: %s\n", w->device, w->error);
		w->failed = 1;
		gpuThreadDone(w);
		return NULL;
	}
	warmUp(w->ctx, w->fb, &p, w->device);
	crh_tile *share = NULL;
	const uint32_t n = gpuShare(r, w->device, G, &share);
	uint64_t pixels = 0;
	for (uint32_t i = 0; i < n; ++i) pixels += (uint64_t)(share[i].x1 - share[i].x0) * (uint64_t)(share[i].y1 - share[i].y0);
	w->state->currentTileNum = 0;
	w->uploadUs = getUs(phase);
	w->readyUs = getUs(w->frameStart);
	startTimer(&phase);
	int passes = r->prefs.sampleCount;
	if (pixels && (uint64_t)passes * pixels > FIRST_DISPATCH_PATHS) passes = (int)(FIRST_DISPATCH_PATHS / pixels);
	const int fixedPasses = getenv("CRH_DROPIN_PASSES") ? atoi(getenv("CRH_DROPIN_PASSES")) : 0;          /* dev / tests: that many passes per dispatch */
	if (fixedPasses > 0) passes = fixedPasses;
	if (passes < 1) passes = 1;
	if (adapt && n) {
		/* the whole frame in one call: the library's loop renders, measures and decides, rectangle by rectangle (no preview, no pause in between) */
		w->adaptCount = adaptiveRectangles(r, share, n, G, &w->adaptTiles);
		w->adaptUnits = w->adaptCount;
		crh_adaptive_cells_params cells;
		crh_adaptive_cells_params_default(&cells);
		cells.min_passes = adaptive.min_passes; cells.threshold = adaptive.threshold;
		if (w->adaptTiles && adaptiveCellSettings(&cells.cell, &cells.dilate) > 0) {
			const int64_t total = crh_adaptive_cell_offsets(w->adaptTiles, w->adaptCount, cells.cell, NULL);
			if (total >= 0) { w->adaptCell = cells.cell; w->adaptUnits = (uint32_t)total; }
			else logr(warning, "GPU %d: CRAY_HIP_ADAPTIVE_CELL=%i: %s; deciding per rectangle\n", w->device, cells.cell, crh_last_error());
		}
		w->adaptPasses = calloc(w->adaptUnits ? w->adaptUnits : 1, sizeof(*w->adaptPasses));
		p.first_pass = 0; p.pass_count = r->prefs.sampleCount;
		struct timeval tl;
		startTimer(&tl);
		const int rc = !w->adaptTiles || !w->adaptPasses ? CRH_ERR_NOMEM
			: w->adaptCell ? crh_render_adaptive_cells(w->ctx, &p, w->adaptTiles, w->adaptCount, &cells, w->fb, w->half, w->adaptPasses, NULL)
			: crh_render_adaptive(w->ctx, &p, w->adaptTiles, w->adaptCount, &adaptive, w->fb, w->half, w->adaptPasses, NULL);
		w->launchUs += getUs(tl);
		announceLaunch(w);
		if (rc != CRH_OK || crh_synchronize(w->ctx) != CRH_OK) {
			snprintf(w->error, sizeof(w->error), "%s", rc == CRH_ERR_NOMEM ? "out of memory" : crh_last_error());
			logr(warning, "GPU %d: %s\n", w->device, w->error);
			w->failed = 1;
		} else {
			w->dispatches++;
			w->state->completedSamples = r->prefs.sampleCount;
			w->state->totalSamples = pixels * (uint64_t)r->prefs.sampleCount;
		}
	}
	for (int done = adapt ? r->prefs.sampleCount : 0; done < r->prefs.sampleCount && r->state.isRendering && !r->state.renderAborted; ) {
		p.first_pass = done;
		p.pass_count = r->prefs.sampleCount - done < passes ? r->prefs.sampleCount - done : passes;
		if (done < halfAt && done + p.pass_count > halfAt) p.pass_count = halfAt - done;          /* a dispatch ends exactly where the copy is taken */
		struct timeval tl;
		startTimer(&tl);
		int rc = n ? crh_render_tiles(w->ctx, &p, share, n, w->fb) : CRH_OK;
		w->launchUs += getUs(tl);
		announceLaunch(w);
		if (n && (rc != CRH_OK || crh_synchronize(w->ctx) != CRH_OK)) {
			snprintf(w->error, sizeof(w->error), "%s", crh_last_error());
			logr(warning, "GPU %d: %s\n", w->device, w->error);
			w->failed = 1;
			break;
		}
		const long us = getUs(tl);
		w->dispatches++;
		done += p.pass_count;
		w->state->completedSamples = done;
		w->state->totalSamples = pixels * (uint64_t)done;
		if (halfAt && done == halfAt && crh_framebuffer_copy(w->ctx, w->fb, w->half, W, H) != CRH_OK) {          /* (in stream order: before the next dispatch folds into fb) */
			snprintf(w->error, sizeof(w->error), "%s", crh_last_error());
			logr(warning, "GPU %d: %s\n", w->device, w->error);
			w->failed = 1;
			break;
		}
		if (done < r->prefs.sampleCount) {
			/* more to come: show what there is, and size the next dispatch by what this one cost */
			if (n && refreshOutput(w->ctx, w->fb, W, H, w->output, w->device, G) != CRH_OK) logr(warning, "GPU %d: preview: %s\n", w->device, crh_last_error());
			const double msPerPass = (double)us / 1e3 / (double)p.pass_count;
			passes = msPerPass > 0.0 ? (int)(DISPATCH_TARGET_MS / msPerPass) : passes;
			if (fixedPasses > 0) passes = fixedPasses;
			if (passes < 1) passes = 1;
		}
		while (w->state->paused && !r->state.renderAborted) sleepMSec(100);
	}
	w->renderUs = getUs(phase);
	crh_counters c;
	if (!w->failed && crh_counters_get(w->ctx, &c) == CRH_OK) w->rays = c.rays;
	{ float last = 0.0f; uint64_t launches = 0; if (!w->failed) crh_kernel_time_ms(w->ctx, &last, &w->kernelMs, &launches); }
	free(share);
	gpuThreadDone(w);
	return NULL;
}

struct commWarm { int devices[MAX_GPUS]; int n; int rc; long us; };
static void *commThread(void *arg) {
	struct commWarm *cw = threadUserData(arg);
	struct timeval t;
	startTimer(&t);
	cw->rc = crh_frames_prepare(cw->devices, cw->n);
	cw->us = getUs(t);
	return NULL;
}

/* the G per-GPU framebuffers -> GPU 0's: the strips (1 / G of the frame per link), or — CRH_FRAMES=reduce, or a librccl without send / receive — one ncclReduce */
static void assembleFrame(crh_ctx **ctxs, float **fbs, int gpus, int W, int H) {
	if (gpus < 2) return;
	const char *how = getenv("CRH_FRAMES");
	int rc = (how && !strcmp(how, "reduce")) ? CRH_ERR_UNSUPPORTED : crh_frames_gather(ctxs, fbs, gpus, W, H, CRH_STRIP_ROWS);
	if (rc == CRH_ERR_UNSUPPORTED) rc = crh_frames_reduce(ctxs, fbs, gpus, W, H);
	if (rc != CRH_OK) logr(error, "c-ray-hip: assembling the frame on GPU 0 failed: %s\n", crh_last_error());
}

/* --iterative: returns the rays traced, fills state.renderBuffer and output */
static uint64_t renderInteractive(struct renderer *r, struct texture *output, const crh_scene_desc *scene, int gpus) {
	const int W = (int)r->prefs.imageWidth, H = (int)r->prefs.imageHeight;
	crh_ctx *ctx[MAX_GPUS];
	float *fb[MAX_GPUS];
	crh_tile *tiles[MAX_GPUS];
	uint32_t ntiles[MAX_GPUS];
	/* the process's pooled contexts (round 5, ADVICE r04: this mode used to create a second context per GPU beside the pool's); several GPUs: one layout compile */
	crh_compiled_scene *compiled = NULL;
	if (gpus > 1 && crh_scene_compile(scene, frameWalk(), &compiled) != CRH_OK) logr(error, "c-ray-hip: %s\n", crh_last_error());          /* (the pooled contexts' CRH_OPT_WALK; the Halton sampler keeps the binary walk either way) */
	for (int g = 0; g < gpus; ++g) {
		ctx[g] = poolAcquire(g);
		if (!ctx[g] || crh_counters_reset(ctx[g]) != CRH_OK || crh_set_option(ctx[g], CRH_OPT_SAMPLER, CRH_SAMPLER_HALTON) != CRH_OK ||
			crh_set_option(ctx[g], CRH_OPT_COUNTER_LEVEL, 1) != CRH_OK || (compiled ? crh_scene_upload_compiled(ctx[g], compiled) : crh_scene_upload(ctx[g], scene)) != CRH_OK ||
			crh_framebuffer_alloc(ctx[g], W, H, &fb[g]) != CRH_OK)
			logr(error, "c-ray-hip: GPU %i: %s\n", g, crh_last_error());
		ntiles[g] = gpuShare(r, g, gpus, &tiles[g]);
	}
	crh_compiled_scene_free(compiled);
	const int passes = r->prefs.sampleCount - 1;             /* finishedPasses runs from 1 while < sampleCount (renderer.c:199, tile.c:52) */
	crh_render_params p;
	memset(&p, 0, sizeof(p));
	p.image_width = W; p.image_height = H; p.max_passes = r->prefs.sampleCount; p.bounces = r->prefs.bounces;
	for (int g = 0; g < gpus; ++g) warmUp(ctx[g], fb[g], &p, g);
	int done = 0;
	int chunk = 1;                                           /* the first preview after one pass; then as many passes per dispatch as take about a display refresh */
	int dispatches = 0;
	struct timeval loop;
	startTimer(&loop);
	while (done < passes && !r->state.renderAborted) {
		if (chunk > passes - done) chunk = passes - done;
		p.first_pass = done; p.pass_count = chunk;
		struct timeval tc;
		startTimer(&tc);
		for (int g = 0; g < gpus; ++g)
			if (ntiles[g] && crh_render_tiles(ctx[g], &p, tiles[g], ntiles[g], fb[g]) != CRH_OK) logr(error, "c-ray-hip: GPU %i: %s\n", g, crh_last_error());
		/* the 8-bit frame of this chunk, converted where the float buffer lives (stream order: after the chunk's kernel) */
		for (int g = 0; g < gpus; ++g)
			if (ntiles[g] && refreshOutput(ctx[g], fb[g], W, H, output, g, gpus) != CRH_OK) logr(error, "c-ray-hip: GPU %i: %s\n", g, crh_last_error());
		const double chunkMs = (double)getUs(tc) / 1e3;
		done += chunk;
		++dispatches;
		r->state.finishedPasses = done + 1;
		for (int g = 0; g < gpus; ++g) {
			r->state.threadStates[g].completedSamples = done;
			r->state.threadStates[g].totalSamples += (uint64_t)chunk;
		}
		getKeyboardInput(r);
		drawWindow(r, output);
		while (r->state.threadStates[0].paused && !r->state.renderAborted) { getKeyboardInput(r); sleepMSec(100); }
		/* ~16 ms of GPU work between two redraws: the host side of a chunk (launch, 8-bit download, redraw) stays a small part of it */
		const double msPerPass = chunkMs / (double)chunk;
		int next = msPerPass > 0.0 ? (int)(16.0 / msPerPass) : chunk;
		if (next > 2 * chunk) next = 2 * chunk;              /* grow gently: the first passes' previews are the ones a user watches */
		chunk = next < 1 ? 1 : (next > 256 ? 256 : next);
	}
	const long loopUs = getUs(loop);
	/* CRH_DUMP_STATS: how busy the GPU was while the frame converged (kernel time of GPU 0 / wall time of the loop: launches, 8-bit downloads, redraws are the rest) */
	const char *statsPath = getenv("CRH_DUMP_STATS");
	if (statsPath) {
		double kernelMs = 0.0;
		float last = 0.0f;
		uint64_t launches = 0;
		crh_kernel_time_ms(ctx[0], &last, &kernelMs, &launches);
		FILE *f = fopen(statsPath, "w");
		if (f) {
			fprintf(f, "{\"mode\": \"iterative\", \"gpus\": %d, \"width\": %d, \"height\": %d, \"passes\": %d, \"dispatches\": %d, \"loop_ms\": %.3f, \"kernel_ms\": %.3f, \"gpu_busy\": %.4f}\n",
					gpus, W, H, done, dispatches, loopUs / 1e3, kernelMs, loopUs > 0 ? kernelMs / (loopUs / 1e3) : 0.0);
			fclose(f);
		}
	}
	/* the float buffer: once, at the end */
	assembleFrame(ctx, fb, gpus, W, H);
	if (crh_framebuffer_download(ctx[0], fb[0], W, H, r->state.renderBuffer->data.float_p) != CRH_OK) logr(error, "c-ray-hip: download: %s\n", crh_last_error());
	uint64_t rays = 0;
	for (int g = 0; g < gpus; ++g) {
		crh_counters c;
		if (crh_counters_get(ctx[g], &c) == CRH_OK) rays += c.rays;
		crh_framebuffer_free(ctx[g], fb[g]);
		poolRelease(g, ctx[g], crh_set_option(ctx[g], CRH_OPT_SAMPLER, CRH_SAMPLER_RANDOM) == CRH_OK);          /* (back to the pool as it came: the frame renderer's sampler) */
		free(tiles[g]);
		r->state.threadStates[g].threadComplete = true;
	}
	return rays;
}

/* The strips of the GPUs that failed, rendered by the ones that did not (tile.c:31-42 is the reference's version of this: a lost worker's tiles are handed out
 * again). Strip i of the frame belongs to GPU i mod G (share.h); the strips of a failed GPU are dealt round-robin to the survivors, which render them for ALL
 * passes into their own (there still zero) framebuffers, whatever the failed GPU had got done. Returns 0, or -1 with the survivor's message logged. */
static int redealFailedShares(struct renderer *r, struct gpuWorker *workers, int gpus) {
	const int W = (int)r->prefs.imageWidth, H = (int)r->prefs.imageHeight;
	int survivors[MAX_GPUS], ns = 0;
	for (int g = 0; g < gpus; ++g) if (!workers[g].failed) survivors[ns++] = g;
	if (!ns) return -1;
	crh_tile *extra[MAX_GPUS];
	uint32_t nExtra[MAX_GPUS];
	const size_t cap = (size_t)crh_strip_share_max(H, gpus) * (size_t)gpus;
	for (int s = 0; s < ns; ++s) { extra[s] = calloc(cap ? cap : 1, sizeof(crh_tile)); nExtra[s] = 0; }
	int next = 0, strips = 0;
	for (int g = 0; g < gpus; ++g) {
		if (!workers[g].failed) continue;
		crh_tile *t = NULL;
		const uint32_t n = gpuShare(r, g, gpus, &t);
		for (uint32_t i = 0; i < n; ++i, ++strips) { extra[next][nExtra[next]++] = t[i]; next = (next + 1) % ns; }
		free(t);
	}
	logr(warning, "c-ray-hip: re-dealing the %i strips of the failed GPUs to the %i remaining GPU%s\n", strips, ns, PLURAL(ns));
	crh_render_params p;
	memset(&p, 0, sizeof(p));
	p.image_width = W; p.image_height = H; p.max_passes = r->prefs.sampleCount; p.bounces = r->prefs.bounces;
	uint64_t most = 1;
	for (int s = 0; s < ns; ++s) {
		uint64_t px = 0;
		for (uint32_t i = 0; i < nExtra[s]; ++i) px += (uint64_t)(extra[s][i].x1 - extra[s][i].x0) * (uint64_t)(extra[s][i].y1 - extra[s][i].y0);
		if (px > most) most = px;
	}
	int passes = r->prefs.sampleCount;
	if ((uint64_t)passes * most > FIRST_DISPATCH_PATHS) passes = (int)(FIRST_DISPATCH_PATHS / most);
	if (passes < 1) passes = 1;
	int rc = 0;
	for (int done = 0; done < r->prefs.sampleCount && !rc && !r->state.renderAborted; done += p.pass_count) {
		p.first_pass = done;
		p.pass_count = r->prefs.sampleCount - done < passes ? r->prefs.sampleCount - done : passes;
		for (int s = 0; s < ns && !rc; ++s)          /* every survivor's dispatch is in flight before the first one is waited for */
			if (nExtra[s] && crh_render_tiles(workers[survivors[s]].ctx, &p, extra[s], nExtra[s], workers[survivors[s]].fb) != CRH_OK) rc = -1;
		for (int s = 0; s < ns && !rc; ++s)
			if (nExtra[s] && crh_synchronize(workers[survivors[s]].ctx) != CRH_OK) rc = -1;
		if (rc) logr(warning, "c-ray-hip: re-dealt strips: %s\n", crh_last_error());
		getKeyboardInput(r);
	}
	for (int s = 0; s < ns; ++s) {
		crh_counters c;
		if (!rc && crh_counters_get(workers[survivors[s]].ctx, &c) == CRH_OK) workers[survivors[s]].rays = c.rays;
		free(extra[s]);
	}
	return rc;
}

/* The frame of a run that lost a GPU: the survivors' float buffers merged on the host (one owner per pixel, 0.0f everywhere else), and the 8-bit output the way
 * renderer.c:296-300 makes it, pixel by pixel, with the reference's own colorToSRGB / setPixel. */
static int assembleOnHost(struct renderer *r, struct gpuWorker *workers, int gpus, struct texture *output) {
	const int W = (int)r->prefs.imageWidth, H = (int)r->prefs.imageHeight;
	float *dst = r->state.renderBuffer->data.float_p;
	float *tmp = malloc((size_t)W * H * 3 * sizeof(float));
	if (!tmp) return -1;
	memset(dst, 0, (size_t)W * H * 3 * sizeof(float));
	for (int g = 0; g < gpus; ++g) {
		if (workers[g].failed) continue;
		if (crh_framebuffer_download(workers[g].ctx, workers[g].fb, W, H, tmp) != CRH_OK) { free(tmp); return -1; }
		for (size_t i = 0; i < (size_t)W * H * 3; ++i) if (tmp[i] != 0.0f) dst[i] = tmp[i];
	}
	free(tmp);
	for (int y = 0; y < H; ++y)
		for (int x = 0; x < W; ++x)
			setPixel(output, colorToSRGB(textureGetPixel(r->state.renderBuffer, x, y, false)), x, y);
	return 0;
}

/* CRAY_HIP_AOV=<n>: min(n, sampleCount) passes of the first-hit buffers of the whole image, on GPU 0 (primary rays only: nothing to gather), written as 8-bit
 * images <imgFileName>_albedo, _normal (0.5 n + 0.5) and _depth (divided by the frame's largest depth) beside the frame, by the reference's own newImageFile /
 * writeImage; CRH_DUMP_AOV_F32=<path> dumps the raw [H, W, 8] floats the way CRH_DUMP_F32 dumps the frame. The scene is still resident in ctx. */
/* `keep` (CRAY_HIP_EXR): where the device buffer goes instead of being freed — it is the caller's then. */
static void writeAovs(struct renderer *r, crh_ctx *ctx, int W, int H, float **keep) {
	const char *e = getenv("CRAY_HIP_AOV");
	int n = e ? atoi(e) : 0;
	if (n <= 0 || !ctx) return;
	if (n > r->prefs.sampleCount) n = r->prefs.sampleCount;
	const size_t pixels = (size_t)W * (size_t)H;
	float *host = malloc(pixels * CRH_AOV_CHANNELS * sizeof(float));
	float *dev = NULL;
	crh_render_params p;
	memset(&p, 0, sizeof(p));
	p.x1 = W; p.y1 = H; p.image_width = W; p.image_height = H; p.pass_count = n; p.max_passes = r->prefs.sampleCount;
	if (!host || crh_aov_alloc(ctx, W, H, &dev) != CRH_OK || crh_render_aov(ctx, &p, NULL, 0, dev) != CRH_OK || crh_aov_download(ctx, dev, W, H, host) != CRH_OK) {
		logr(warning, "c-ray-hip: the AOV buffers could not be rendered: %s\n", host ? crh_last_error() : "out of memory");
		if (dev) crh_aov_free(ctx, dev);
		free(host);
		return;
	}
	if (keep) *keep = dev;
	else crh_aov_free(ctx, dev);
	const char *dump = getenv("CRH_DUMP_AOV_F32");
	if (dump) {
		FILE *f = fopen(dump, "wb");
		if (f) { fwrite(host, sizeof(float), pixels * CRH_AOV_CHANNELS, f); fclose(f); }
	}
	float maxDepth = 0.0f;
	for (size_t i = 0; i < pixels; ++i) if (host[i * CRH_AOV_CHANNELS + 6] > maxDepth) maxDepth = host[i * CRH_AOV_CHANNELS + 6];
	static const char *const suffix[3] = {"_albedo", "_normal", "_depth"};
	const char *base = r->prefs.imgFileName ? r->prefs.imgFileName : "rendered";
	for (int k = 0; k < 3; ++k) {
		struct texture *t = newTexture(char_p, (size_t)W, (size_t)H, 3);
		for (size_t i = 0; i < pixels; ++i) {          /* (the buffer's pixel order is the frame's: texture.c:24-28) */
			const float *a = host + i * CRH_AOV_CHANNELS;
			for (int c = 0; c < 3; ++c) {
				float v = k == 0 ? a[c] : k == 1 ? 0.5f * a[3 + c] + 0.5f : (maxDepth > 0.0f ? a[6] / maxDepth : 0.0f);
				v = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;          /* (NaN -> 0) */
				t->data.byte_p[i * 3 + (size_t)c] = (unsigned char)(v * 255.0f);
			}
		}
		char *name = malloc(strlen(base) + strlen(suffix[k]) + 1);
		if (name) {
			strcpy(name, base); strcat(name, suffix[k]);
			struct imageFile *file = newImageFile(t, r->prefs.imgFilePath ? r->prefs.imgFilePath : "", name, r->prefs.imgCount, r->prefs.imgType);
			writeImage(file);
			destroyImageFile(file);          /* (the texture goes with it) */
			free(name);
		} else destroyTexture(t);
	}
	logr(info, "%i AOV pass%s written (albedo, normal, depth).\n", n, n == 1 ? "" : "es");
	free(host);
}

/* CRAY_HIP_DENOISE=<iterations, 1..8>: the frame on GPU 0, filtered by crh_denoise — with `half`, the frame after its first halfPasses passes, by
 * crh_denoise_variance (CRAY_HIP_DENOISE_VARIANCE=1) — into a second buffer with guides rendered here — CRAY_HIP_AOV's n passes if that
 * is set, min(16, sampleCount) otherwise —, written as <imgFileName>_denoised beside the frame (8-bit exactly as the frame's: crh_framebuffer_to_srgb8, then the
 * reference's newImageFile / writeImage); CRH_DUMP_DENOISED_F32=<path> dumps the [H, W, 3] floats. Unset: nothing is allocated, nothing is written. */
/* CRAY_HIP_DESPECKLE=<factor> beside CRAY_HIP_DENOISE (CRAY_HIP_DESPECKLE_RANK / _RADIUS / _FLOOR beside it; crx_despeckle's defaults otherwise): the denoiser's
 * input becomes a despeckled COPY of the frame — fireflies scaled down to factor * a rank of their neighbourhood + floor (include/cray_hip_exr.h) —, and with
 * `half` a copy of the half-sample frame under the same plane. The copies are the caller's to free (crh_framebuffer_free). The frame and `half` are only read.
 * False — unset, a bad value (a warning), or a failure (a warning) —: no copy is left behind and the denoiser takes the frame as it is. */
static bool despeckledCopies(crh_ctx *ctx, const float *fb, const float *half, int W, int H, float **fbCopy, float **halfCopy) {
	const char *envFactor = getenv("CRAY_HIP_DESPECKLE"), *envRank = getenv("CRAY_HIP_DESPECKLE_RANK"), *envRadius = getenv("CRAY_HIP_DESPECKLE_RADIUS"),
	           *envFloor = getenv("CRAY_HIP_DESPECKLE_FLOOR");
	if (!envFactor) return false;
	crx_despeckle_params p;
	crx_despeckle_default(&p);
	char *end = NULL;
	p.factor = strtof(envFactor, &end);
	bool good = end != envFactor && !*end && p.factor >= 1.0f && p.factor <= 0x1p20f;
	if (envRadius) {
		const long v = strtol(envRadius, &end, 10);
		good = good && end != envRadius && !*end && (v == 1 || v == 2);
		p.radius = (int)v;
	}
	if (envRank) {
		const long v = strtol(envRank, &end, 10);
		good = good && end != envRank && !*end && v >= 1 && v <= (2 * p.radius + 1) * (2 * p.radius + 1) - 1;
		p.rank = (int)v;
	}
	if (envFloor) {
		p.floor = strtof(envFloor, &end);
		good = good && end != envFloor && !*end && p.floor >= 0.0f && p.floor <= 0x1p20f;
	}
	if (!good) {
		logr(warning, "c-ray-hip: a bad value among CRAY_HIP_DESPECKLE / _RANK / _RADIUS / _FLOOR; the frame is denoised as it is\n");
		return false;
	}
	const char *why = NULL;
	crx_ctx *zip = NULL;
	crx_despeckle_stats stats;
	float ms[2] = {0.0f, 0.0f};
	bool ok = crh_framebuffer_alloc(ctx, W, H, fbCopy) == CRH_OK && crh_framebuffer_copy(ctx, fb, *fbCopy, W, H) == CRH_OK &&
		(!half || (crh_framebuffer_alloc(ctx, W, H, halfCopy) == CRH_OK && crh_framebuffer_copy(ctx, half, *halfCopy, W, H) == CRH_OK)) &&
		crh_synchronize(ctx) == CRH_OK;          /* the companion's stream is its own: the copies must be complete */
	if (!ok) why = crh_last_error();
	if (ok && crx_context_create(0, NULL, &zip) != CRH_OK) { ok = false; why = crx_last_error(); }
	float *frames[2] = {*fbCopy, *halfCopy};
	if (ok && (crx_despeckle(zip, &p, *fbCopy, W, H, frames, half ? 2u : 1u, &stats) != CRH_OK || crx_despeckle_time_ms(zip, ms) != CRH_OK)) { ok = false; why = crx_last_error(); }
	crx_context_destroy(zip);
	if (ok) {
		logr(info, "Despeckled the denoiser's input (radius %i, rank %i, factor %g, floor %g): %llu pixels clamped, %llu bad, brightest %g, %.3f ms.\n", p.radius, p.rank,
			(double)p.factor, (double)p.floor, (unsigned long long)stats.clamped, (unsigned long long)stats.bad, (double)stats.max_clamped, (double)(ms[0] + ms[1]));
		return true;
	}
	logr(warning, "c-ray-hip: the frame could not be despeckled (%s); it is denoised as it is\n", why ? why : "unknown");
	if (*fbCopy) crh_framebuffer_free(ctx, *fbCopy);
	if (*halfCopy) crh_framebuffer_free(ctx, *halfCopy);
	*fbCopy = *halfCopy = NULL;
	return false;
}

/* `keep` (CRAY_HIP_EXR): where the denoised device buffer goes instead of being freed — it is the caller's then. */
static void writeDenoised(struct renderer *r, crh_ctx *ctx, const float *fb, const float *half, int halfPasses, int W, int H, float **keep) {
	const char *e = getenv("CRAY_HIP_DENOISE");
	const int iterations = e ? atoi(e) : 0;
	if (iterations <= 0 || !ctx || !fb) return;
	const char *v = getenv("CRAY_HIP_DENOISE_VARIANCE");
	if (v && atoi(v) > 0 && !half) logr(warning, "c-ray-hip: CRAY_HIP_DENOISE_VARIANCE needs at least 2 samples to split; using the plain filter\n");
	const char *a = getenv("CRAY_HIP_AOV");
	int n = a ? atoi(a) : 0;
	if (n <= 0) n = 16;
	if (n > r->prefs.sampleCount) n = r->prefs.sampleCount;
	const size_t pixels = (size_t)W * (size_t)H;
	float *aov = NULL, *out = NULL;
	float *host = malloc(pixels * 3 * sizeof(float));
	struct texture *t = newTexture(char_p, (size_t)W, (size_t)H, 3);
	crh_render_params p;
	memset(&p, 0, sizeof(p));
	p.x1 = W; p.y1 = H; p.image_width = W; p.image_height = H; p.pass_count = n; p.max_passes = r->prefs.sampleCount;
	crh_denoise_params d;
	crh_denoise_params_default(&d);
	d.width = W; d.height = H; d.iterations = iterations;
	crh_denoise_variance_params dv;
	crh_denoise_variance_params_default(&dv, halfPasses, r->prefs.sampleCount);
	dv.width = W; dv.height = H; dv.iterations = iterations;
	float ms = 0.0f;
	float *cleanFb = NULL, *cleanHalf = NULL;          /* CRAY_HIP_DESPECKLE: the filter reads despeckled copies; the frame stays as it is */
	if (host && despeckledCopies(ctx, fb, half, W, H, &cleanFb, &cleanHalf)) {
		fb = cleanFb;
		if (half) half = cleanHalf;
	}
	const bool ok = host && crh_aov_alloc(ctx, W, H, &aov) == CRH_OK && crh_framebuffer_alloc(ctx, W, H, &out) == CRH_OK && crh_render_aov(ctx, &p, NULL, 0, aov) == CRH_OK
		&& (half ? crh_denoise_variance(ctx, &dv, fb, half, aov, out) : crh_denoise(ctx, &d, fb, aov, out)) == CRH_OK && crh_denoise_time_ms(ctx, &ms) == CRH_OK && crh_framebuffer_to_srgb8(ctx, out, W, H, t->data.byte_p) == CRH_OK
		&& crh_framebuffer_download(ctx, out, W, H, host) == CRH_OK;
	if (!ok) logr(warning, "c-ray-hip: the frame could not be denoised: %s\n", host ? crh_last_error() : "out of memory");
	if (aov) crh_aov_free(ctx, aov);
	if (cleanFb) crh_framebuffer_free(ctx, cleanFb);
	if (cleanHalf) crh_framebuffer_free(ctx, cleanHalf);
	if (out && ok && keep) *keep = out;
	else if (out) crh_framebuffer_free(ctx, out);
	const char *base = r->prefs.imgFileName ? r->prefs.imgFileName : "rendered";
	char *name = ok ? malloc(strlen(base) + strlen("_denoised") + 1) : NULL;
	if (name) {
		const char *dump = getenv("CRH_DUMP_DENOISED_F32");
		if (dump) {
			FILE *f = fopen(dump, "wb");
			if (f) { fwrite(host, sizeof(float), pixels * 3, f); fclose(f); }
		}
		strcpy(name, base); strcat(name, "_denoised");
		struct imageFile *file = newImageFile(t, r->prefs.imgFilePath ? r->prefs.imgFilePath : "", name, r->prefs.imgCount, r->prefs.imgType);
		writeImage(file);
		destroyImageFile(file);          /* (the texture goes with it) */
		free(name);
		logr(info, "Denoised frame written (%s%i iteration%s, %i guide pass%s, %.3f ms).\n", half ? "variance-guided, " : "", iterations, iterations == 1 ? "" : "s", n, n == 1 ? "" : "es", (double)ms);
	} else destroyTexture(t);
	free(host);
}

/* CRAY_HIP_EXR=1: the names of the scene's ids, taken while the flattened scene is there (a long frame gives it back early): instance i is <mesh name>#<i> for a mesh
 * instance and sphere#<i> otherwise, material i is material#<i>. */
struct layerNames { char **instances, **materials; uint32_t instanceCount, materialCount; };
static char *numberedName(const char *stem, uint32_t i) {
	char *s = malloc(strlen(stem) + 16);
	if (s) sprintf(s, "%s#%u", stem, i);
	return s;
}
static void layerNamesCollect(const struct renderer *r, const crh_scene_desc *scene, struct layerNames *out) {
	out->instanceCount = (uint32_t)scene->instance_count;
	out->materialCount = (uint32_t)scene->material_count;
	out->instances = calloc(out->instanceCount ? out->instanceCount : 1, sizeof(char *));
	out->materials = calloc(out->materialCount ? out->materialCount : 1, sizeof(char *));
	for (uint32_t i = 0; out->instances && i < out->instanceCount; ++i) {
		const crh_instance *fi = &scene->instances[i];
		const bool mesh = fi->kind == CRH_INSTANCE_MESH || fi->kind == CRH_INSTANCE_MESH_VOLUME;
		const char *name = mesh ? r->scene->meshes[fi->object].name : "sphere";
		out->instances[i] = numberedName(name ? name : "mesh", i);
	}
	for (uint32_t i = 0; out->materials && i < out->materialCount; ++i) out->materials[i] = numberedName("material", i);
}
static void layerNamesFree(struct layerNames *n) {
	for (uint32_t i = 0; n->instances && i < n->instanceCount; ++i) free(n->instances[i]);
	for (uint32_t i = 0; n->materials && i < n->materialCount; ++i) free(n->materials[i]);
	free(n->instances); free(n->materials);
	memset(n, 0, sizeof(*n));
}

/* CRAY_HIP_EXR=1: <imgFilePath><imgFileName>_layers_<imgCount, four digits>.exr — the name the frame's own file would get for <imgFileName>_layers — holds the frame
 * `fb`, the guide buffers `aov` and the denoised frame `denoised` where CRAY_HIP_AOV / CRAY_HIP_DENOISE left them on GPU 0, and with CRAY_HIP_IDS=<n> the ranked ids of
 * min(n, sampleCount) passes of both ID buffers rendered here, as Cryptomatte layers. The channels are packed on the device (crh_pack_scanlines), at most 32 MB a call;
 * with CRAY_HIP_EXR_COMPRESSION=zip|zips beside it they are deflated there as well (crx_pack of libcray_hip_exr.so) and the file is a ZIP / ZIPS one; with
 * CRAY_HIP_EXR_HALF=1 the colour layers are HALF (crx_pack too, whatever the compression); with CRAY_HIP_EXR_CODES=dynamic the deflate blocks may use dynamic Huffman
 * codes (crx_set_codes; anything else or unset: the fixed codes). */
static void writeLayers(struct renderer *r, crh_ctx *ctx, const float *fb, const float *aov, const float *denoised, const struct layerNames *names, int W, int H) {
	const char *e = getenv("CRAY_HIP_IDS");
	int n = e ? atoi(e) : 0;
	if (n > r->prefs.sampleCount) n = r->prefs.sampleCount;
	const bool ids = n > 0 && names->instances && names->materials && names->instanceCount && names->materialCount && names->instanceCount <= 65536 && names->materialCount <= 65536;
	if (n > 0 && !ids) logr(warning, "c-ray-hip: CRAY_HIP_IDS needs 1 .. 65536 instances and materials; the layers file gets no id layers\n");
	uint32_t *buf[2] = {NULL, NULL}, *map[2] = {NULL, NULL};
	float *ranked[2] = {NULL, NULL};          /* [H, W, 6, 2] floats in an ID buffer's 16 words a pixel */
	struct exr_attr strings[8];
	int stringCount = 0;
	bool ok = true;
	if (ids) {
		crh_render_params p;
		memset(&p, 0, sizeof(p));
		p.x1 = W; p.y1 = H; p.image_width = W; p.image_height = H; p.pass_count = n; p.max_passes = r->prefs.sampleCount;
		for (int k = 0; k < 2; ++k) ok = ok && crh_ids_alloc(ctx, W, H, &buf[k]) == CRH_OK && crh_ids_alloc(ctx, W, H, (uint32_t **)&ranked[k]) == CRH_OK;
		ok = ok && crh_render_ids(ctx, &p, NULL, 0, buf[0], buf[1]) == CRH_OK;
		for (int k = 0; k < 2 && ok; ++k) {
			char **list = k ? names->materials : names->instances;
			const uint32_t count = k ? names->materialCount : names->instanceCount;
			ok = crh_ids_resolve(ctx, buf[k], W, H, ranked[k]) == CRH_OK && (map[k] = malloc(count * sizeof(uint32_t))) != NULL;
			for (uint32_t i = 0; ok && i < count; ++i) ok = list[i] != NULL;
			for (uint32_t i = 0; ok && i < count; ++i) map[k][i] = exr_crypto_id(list[i]);
			if (ok && exr_crypto_attrs(k ? "CryptoMaterial" : "CryptoObject", (const char *const *)list, count, strings + stringCount) == 0) stringCount += 4;
			else ok = false;
		}
	}
	crh_pack_channel channels[CRH_PACK_MAX_CHANNELS];
	const char *channelNames[CRH_PACK_MAX_CHANNELS];
	const int count = exr_layer_channels(fb, aov, denoised, ids ? ranked[0] : NULL, ids ? ranked[1] : NULL, map[0], names->instanceCount, map[1], names->materialCount, channels, channelNames);
	/* CRAY_HIP_EXR_COMPRESSION=zip|zips: the chunks deflated on the device by the companion library (crx_pack, include/cray_hip_exr.h), 16 rows or one a chunk */
	const char *how = getenv("CRAY_HIP_EXR_COMPRESSION");
	int kind = 0;
	if (how && !strcmp(how, "zip")) kind = 3;
	else if (how && !strcmp(how, "zips")) kind = 2;
	else if (how && *how && strcmp(how, "none")) logr(warning, "c-ray-hip: CRAY_HIP_EXR_COMPRESSION=%s is not zip, zips or none; the layers file stays uncompressed\n", how);
	const char *halfEnv = getenv("CRAY_HIP_EXR_HALF");
	uint8_t types[CRH_PACK_MAX_CHANNELS];
	const bool half = halfEnv && !strcmp(halfEnv, "1") && exr_half_types(channelNames, count, types) > 0;
	const bool companion = kind || half;          /* crx_pack packs; the uncompressed all-FLOAT file needs crh_pack_scanlines alone */
	const int lines = kind == 3 ? 16 : 1, chunks = (H + lines - 1) / lines;
	const size_t block = 8u + 4u * (size_t)count * (size_t)W;          /* a FLOAT row behind its header: no row of any file takes more */
	char *blocks = ok ? malloc(block * (size_t)H) : NULL;
	uint64_t *sizes = malloc((size_t)chunks * sizeof(*sizes));
	int chunk = (int)(((size_t)32 << 20) / block);
	if (chunk < 1) chunk = 1;
	chunk = (chunk + lines - 1) / lines * lines;
	ok = ok && blocks && sizes;
	const char *why = NULL;
	if (companion && ok) {
		crx_ctx *zip = NULL;
		size_t at = 0;
		ok = crh_synchronize(ctx) == CRH_OK;          /* the companion's stream is its own: the sources must be complete */
		if (ok && crx_context_create(0, NULL, &zip) != CRH_OK) { ok = false; why = crx_last_error(); }
		const char *codes = getenv("CRAY_HIP_EXR_CODES");          /* dynamic: per segment the cheaper of the fixed and a dynamic Huffman code */
		if (ok && codes && !strcmp(codes, "dynamic") && crx_set_codes(zip, CRX_CODES_DYNAMIC) != CRH_OK) { ok = false; why = crx_last_error(); }
		for (int y = 0; ok && y < H; y += chunk) {
			uint64_t total = 0;
			const int rows = H - y < chunk ? H - y : chunk;
			if (crx_pack(zip, channels, half ? types : NULL, (uint32_t)count, W, H, y, rows, kind, blocks + at, sizes + y / lines, &total) != CRH_OK) { ok = false; why = crx_last_error(); }
			at += (size_t)total;
		}
		if (why) logr(warning, "c-ray-hip: %s\n", why);
		crx_context_destroy(zip);
	}
	for (int y = 0; !companion && ok && y < H; y += chunk)
		ok = crh_pack_scanlines(ctx, channels, (uint32_t)count, W, H, y, H - y < chunk ? H - y : chunk, blocks + block * (size_t)y) == CRH_OK;
	for (int y = 0; !companion && ok && y < H; ++y) sizes[y] = block;
	const char *base = r->prefs.imgFileName ? r->prefs.imgFileName : "rendered";
	const char *dir = r->prefs.imgFilePath ? r->prefs.imgFilePath : "";
	char *path = malloc(strlen(dir) + strlen(base) + 32);
	if (ok && path) {
		sprintf(path, "%s%s_layers_%04d.exr", dir, base, r->prefs.imgCount);
		if (exr_write_file(path, W, H, channelNames, half ? types : NULL, count, strings, stringCount, kind, blocks, sizes, chunks) == 0) logr(info, "Layers written to %s (%i channels%s).\n", path, count, ids ? ", Cryptomatte ids" : "");
		else logr(warning, "c-ray-hip: the layers file %s could not be written\n", path);
	} else logr(warning, "c-ray-hip: the layers file could not be made: %s\n", blocks && path && sizes ? crh_last_error() : "out of memory");
	free(sizes);
	free(path); free(blocks);
	exr_free_attrs(strings, stringCount);
	for (int k = 0; k < 2; ++k) {
		if (buf[k]) crh_ids_free(ctx, buf[k]);
		if (ranked[k]) crh_ids_free(ctx, (uint32_t *)ranked[k]);
		free(map[k]);
	}
}

/* CRAY_HIP_PNG=1: <imgFilePath><imgFileName>_gpu_<imgCount, four digits>.png — the frame on GPU 0 as a PNG converted, filtered, deflated and check-summed there
 * (crx_png_pack of libcray_hip_exr.so), with the tEXt chunks "C-ray Samples" and "C-ray Bounces". Written next to the frame's own file, not in its place: the
 * reference's writeImage runs untouched. CRAY_HIP_EXR_CODES=fixed applies; otherwise the codes are dynamic. Unset: nothing is allocated or written.
 * CRAY_HIP_PNG_EXPOSURE / _TONEMAP / _WHITE / _DITHER: the display transform (crx_png_pack_display) and, where it is not the identity, the chunk "C-ray Display". */
static void writeGpuPng(struct renderer *r, crh_ctx *ctx, const float *fb, int W, int H) {
	struct timeval t;
	startTimer(&t);
	char samples[32], bounces[32];
	snprintf(samples, sizeof(samples), "%i", r->prefs.sampleCount);
	snprintf(bounces, sizeof(bounces), "%i", r->prefs.bounces);
	char shown[192];
	crx_png_text text[3] = {{"C-ray Samples", samples}, {"C-ray Bounces", bounces}, {"C-ray Display", shown}};
	uint32_t texts = 2;
	/* the display transform: any of the four variables asks for it; a bad value in one of them: a warning and the file without a transform */
	static const char *const curveNames[4] = {"clamp", "reinhard", "aces", "hable"};
	const char *envExposure = getenv("CRAY_HIP_PNG_EXPOSURE"), *envCurve = getenv("CRAY_HIP_PNG_TONEMAP"), *envWhite = getenv("CRAY_HIP_PNG_WHITE"),
	           *envDither = getenv("CRAY_HIP_PNG_DITHER");
	crx_display display;
	crx_display_default(&display);
	const bool autoExposure = envExposure && !strcmp(envExposure, "auto");
	bool transform = envExposure || envCurve || envWhite || envDither, good = true;
	char *end = NULL;
	if (envExposure && !autoExposure) {
		display.exposure = strtof(envExposure, &end);
		good = good && end != envExposure && !*end && display.exposure >= 0x1p-40f && display.exposure <= 0x1p40f;
	}
	if (envCurve) {
		display.curve = -1;
		for (int i = 0; i < 4; ++i) if (!strcmp(envCurve, curveNames[i])) display.curve = i;
		good = good && display.curve >= 0;
	}
	if (envWhite) {
		display.white = strtof(envWhite, &end);
		good = good && end != envWhite && !*end && display.white >= 0x1p-10f && display.white <= 0x1p10f;
	}
	if (envDither) {
		display.dither = !strcmp(envDither, "1");
		good = good && (display.dither || !strcmp(envDither, "0"));
	}
	if (transform && !good) {
		logr(warning, "c-ray-hip: a bad value among CRAY_HIP_PNG_EXPOSURE / _TONEMAP / _WHITE / _DITHER; the GPU PNG is written without a display transform\n");
		transform = false;
	}
	const char *base = r->prefs.imgFileName ? r->prefs.imgFileName : "rendered";
	const char *dir = r->prefs.imgFilePath ? r->prefs.imgFilePath : "";
	const char *codes = getenv("CRAY_HIP_EXR_CODES");
	const char *why = NULL;
	uint64_t bound = 0, total = 0;
	crx_ctx *png = NULL;
	char *path = malloc(strlen(dir) + strlen(base) + 32);
	void *file = NULL;
	bool ok = path != NULL;
	if (ok && crh_synchronize(ctx) != CRH_OK) { ok = false; why = crh_last_error(); }          /* the companion's stream is its own: the frame must be complete */
	if (ok && crx_context_create(0, NULL, &png) != CRH_OK) { ok = false; why = crx_last_error(); }
	if (ok && crx_set_codes(png, codes && !strcmp(codes, "fixed") ? CRX_CODES_FIXED : CRX_CODES_DYNAMIC) != CRH_OK) { ok = false; why = crx_last_error(); }
	if (ok && transform && autoExposure) {          /* the exposure that takes the median luminance to 0.18, measured on the device */
		float key = 0.0f;
		uint64_t counted = 0;
		if (crx_auto_exposure(png, fb, W, H, 500u, 0.18f, &display.exposure, &key, &counted) != CRH_OK) { ok = false; why = crx_last_error(); }
	}
	if (ok && transform && (display.exposure != 1.0f || display.curve != CRX_CURVE_CLAMP || display.dither)) {
		snprintf(shown, sizeof(shown), "exposure=%.9g%s curve=%s white=%.9g dither=%d", (double)display.exposure, autoExposure ? " (auto 500/1000 of 0.18)" : "",
			curveNames[display.curve], (double)display.white, display.dither);
		texts = 3;
		logr(info, "GPU PNG display transform: %s\n", shown);
	}
	if (ok && !(crx_png_bound(W, H, text, texts, &bound) == CRH_OK && (file = malloc((size_t)bound)) != NULL)) { ok = false; why = "out of memory"; }
	if (ok && crx_png_pack_display(png, fb, W, H, transform ? &display : NULL, CRX_PNG_FILTER_ADAPTIVE, text, texts, file, bound, &total) != CRH_OK) { ok = false; why = crx_last_error(); }
	float phases[CRX_PNG_PHASES] = {0};
	if (ok) (void)crx_png_phases_ms(png, phases);
	crx_context_destroy(png);
	if (ok) {
		sprintf(path, "%s%s_gpu_%04d.png", dir, base, r->prefs.imgCount);
		FILE *f = fopen(path, "wb");
		ok = f && fwrite(file, 1, (size_t)total, f) == (size_t)total;
		if (f && fclose(f) != 0) ok = false;
		if (ok) logr(info, "GPU PNG written to %s: %llu bytes, encoded in %.2f ms (kernels %.2f ms).\n", path, (unsigned long long)total, getUs(t) / 1000.0,
			(double)(phases[0] + phases[1] + phases[2] + phases[3] + phases[4]));
		else logr(warning, "c-ray-hip: the GPU PNG %s could not be written\n", path);
	} else logr(warning, "c-ray-hip: the GPU PNG could not be made: %s\n", why ? why : "out of memory");
	free(file);
	free(path);
}

struct texture *renderFrame(struct renderer *r) {
	const int W = (int)r->prefs.imageWidth, H = (int)r->prefs.imageHeight;
	struct timeval frame;
	startTimer(&frame);
	struct texture *output = newTexture(char_p, r->prefs.imageWidth, r->prefs.imageHeight, 3);

	int gpus = crh_device_count();
	const char *cap = getenv("CRAY_HIP_DEVICES");
	if (cap && atoi(cap) > 0 && atoi(cap) < gpus) gpus = atoi(cap);
	if (gpus > MAX_GPUS) gpus = MAX_GPUS;
	if (gpus < 1) logr(error, "c-ray-hip: no HIP device visible (this renderer has no CPU path)\n");

	logr(info, "Starting C-ray MI355X renderer for frame %i\n", r->prefs.imgCount);
	logr(info, "Rendering at %i x %i, %i samples, %i bounces on %i GPU%s.\n", W, H, r->prefs.sampleCount, r->prefs.bounces, gpus, PLURAL(gpus));

	r->state.isRendering = true;
	r->state.renderAborted = false;
	r->state.saveImage = true;
	r->prefs.threadCount = gpus;              /* ui.c indexes threadStates[0..threadCount) */
	r->state.threads = calloc((size_t)gpus, sizeof(*r->state.threads));
	r->state.threadStates = calloc((size_t)gpus, sizeof(*r->state.threadStates));

	/* the RCCL communicators of a multi-GPU frame: created beside everything else, not inside the frame's gather */
	struct commWarm warm = {.n = gpus};
	struct crThread warmThread = {.threadFunc = commThread, .userData = &warm};
	bool warming = false;
	if (gpus > 1) {
		for (int g = 0; g < gpus; ++g) warm.devices[g] = g;
		warming = threadStart(&warmThread) == 0;
	}

	crh_scene_desc scene;
	struct timeval phase;
	if (isSet("interactive")) {
		startTimer(&phase);
		if (crh_flatten_world(r, &scene) != CRH_OK) logr(error, "c-ray-hip: the scene cannot be flattened for the GPU\n");
		logr(info, "Pathtracing iteratively...\n");
		for (int g = 0; g < gpus; ++g)
			r->state.threadStates[g] = (struct renderThreadState){.thread_num = g, .renderer = r, .output = output, .currentTileNum = -1};
		if (warming) threadWait(&warmThread);
		const uint64_t rays = renderInteractive(r, output, &scene, gpus);
		r->state.isRendering = false;
		const char *dumpi = getenv("CRH_DUMP_F32");
		if (dumpi) {
			FILE *f = fopen(dumpi, "wb");
			if (f) { fwrite(r->state.renderBuffer->data.float_p, sizeof(float), (size_t)W * H * 3, f); fclose(f); }
		}
		logr(info, "%llu rays traced on %i GPU%s.\n", (unsigned long long)rays, gpus, PLURAL(gpus));
		crh_flatten_free(&scene);
		return output;
	}
	struct frameSync sync;
	pthread_mutex_init(&sync.mu, NULL);
	pthread_cond_init(&sync.cv, NULL);
	sync.sceneReady = 0; sync.finished = 0; sync.launched = 0; sync.compiled = NULL;
	struct gpuWorker workers[MAX_GPUS];
	memset(workers, 0, sizeof(workers));
	for (int i = 0; i < r->state.tileCount; ++i) r->state.renderTiles[i].isRendering = true;      /* every GPU works on the whole frame (strips): all tiles are "being rendered" until the frame is done */
	for (int g = 0; g < gpus; ++g) {
		r->state.threadStates[g] = (struct renderThreadState){.thread_num = g, .renderer = r, .output = output, .currentTileNum = -1};
		workers[g] = (struct gpuWorker){.r = r, .state = &r->state.threadStates[g], .scene = &scene, .device = g, .sync = &sync, .output = output, .frameStart = frame};
		r->state.threads[g] = (struct crThread){.threadFunc = gpuThread, .userData = &workers[g]};
		if (threadStart(&r->state.threads[g])) logr(error, "Failed to create the dispatch thread of GPU %i.\n", g);
		r->state.activeThreads++;
	}
	/* main thread: flatten the scene while the GPU threads set themselves up */
	startTimer(&phase);
	int frc = crh_flatten_world(r, &scene);
	const long flattenUs = getUs(phase);
	const bool layers = getenv("CRAY_HIP_EXR") && atoi(getenv("CRAY_HIP_EXR")) > 0;
	const bool gpuPng = getenv("CRAY_HIP_PNG") && atoi(getenv("CRAY_HIP_PNG")) > 0;
	struct layerNames layerNames;
	memset(&layerNames, 0, sizeof(layerNames));
	if (layers && frc == CRH_OK) layerNamesCollect(r, &scene, &layerNames);
	/* several GPUs: ONE layout compile, here, behind the flattener; the GPU threads only copy (the reference builds its scene once and every worker reads it:
	 * src/datatypes/scene.c:111-213). One GPU: its crh_scene_upload compiles with the texels' copy beside it */
	crh_compiled_scene *compiled = NULL;
	if (frc == CRH_OK && gpus > 1 && !getenv("CRH_DROPIN_COMPILE_PER_GPU") && crh_scene_compile(&scene, frameWalk(), &compiled) != CRH_OK) {
		logr(warning, "c-ray-hip: %s\n", crh_last_error());
		frc = CRH_ERR_INVALID;
	}
	const long compileUs = getUs(phase) - flattenUs;
	pthread_mutex_lock(&sync.mu);
	sync.compiled = compiled;
	sync.sceneReady = frc == CRH_OK ? 1 : -1;
	pthread_cond_broadcast(&sync.cv);
	pthread_mutex_unlock(&sync.mu);

	/* main thread: keep the preview window / key handling alive while the GPUs work (ui.c contract); a finishing GPU thread wakes it at once */
	for (;;) {
		pthread_mutex_lock(&sync.mu);
		if (sync.finished < gpus) {
			struct timespec until;
			clock_gettime(CLOCK_REALTIME, &until);
			until.tv_nsec += (r->state.renderAborted ? 1 : 16) * 1000000L;
			if (until.tv_nsec >= 1000000000L) { until.tv_sec++; until.tv_nsec -= 1000000000L; }
			pthread_cond_timedwait(&sync.cv, &sync.mu, &until);
		}
		const int finished = sync.finished, launched = sync.launched;
		pthread_mutex_unlock(&sync.mu);
		/* every GPU has its copy of the scene and is busy with its first dispatch: the flattened arrays (70 MB for hdr.json) go back NOW, while this thread has nothing
		 * to do — at the end of renderFrame() the same free() is milliseconds of the frame (a process that has the GPU open gives pages back slowly, and what its threads
		 * launch or wait for meanwhile waits too: only when a GPU's share is long enough to hide it — 2^26 paths, like the library's own release, cray_hip.hip) */
		if (launched == gpus && scene.struct_size && (uint64_t)W * H * (uint64_t)r->prefs.sampleCount / (uint64_t)gpus >= ((uint64_t)1 << 26)) {
			crh_flatten_free(&scene);
			crh_compiled_scene_free(compiled); compiled = NULL;          /* (every GPU thread has announced its launch: the compiled layout has been read for the last time) */
		}
		if (finished == gpus) break;
		getKeyboardInput(r);
		drawWindow(r, output);
	}
	for (int g = 0; g < gpus; ++g) threadWait(&r->state.threads[g]);
	if (warming) threadWait(&warmThread);
	r->state.activeThreads = 0;
	r->state.isRendering = false;
	if (frc != CRH_OK) logr(error, "c-ray-hip: the scene cannot be flattened for the GPU (%i)\n", frc);

	int failed = 0;
	uint64_t rays = 0;
	const char *firstError = "";
	for (int g = gpus - 1; g >= 0; --g) { failed += workers[g].failed; rays += workers[g].rays; if (workers[g].failed) firstError = workers[g].error; }
	if (failed) {
		logr(warning, "c-ray-hip: %i GPU dispatch thread%s failed: %s\n", failed, PLURAL(failed), firstError);
		if (failed == gpus) logr(error, "c-ray-hip: no GPU is left to render the frame: %s\n", firstError);
		if (!r->state.renderAborted && redealFailedShares(r, workers, gpus) != 0) logr(error, "c-ray-hip: the strips of the failed GPU%s could not be rendered elsewhere\n", PLURAL(failed));
		rays = 0;
		for (int g = 0; g < gpus; ++g) if (!workers[g].failed) rays += workers[g].rays;
	}
	if (warming && warm.rc != CRH_OK) logr(warning, "c-ray-hip: RCCL set-up beside the frame failed; the gather will retry\n");
	if (!r->state.renderAborted)
		for (int i = 0; i < r->state.tileCount; ++i) { r->state.renderTiles[i].isRendering = false; r->state.renderTiles[i].renderComplete = true; }

	startTimer(&phase);
	struct texture *buf = r->state.renderBuffer;
	long gatherUs = 0, resolveUs = 0, downloadUs = 0;
	if (failed) {
		/* a GPU was lost: the survivors hold the whole frame between them, but not in the strip pattern the gather moves */
		if (assembleOnHost(r, workers, gpus, output) != 0) logr(error, "c-ray-hip: assembling the frame on the host failed: %s\n", crh_last_error());
		gatherUs = getUs(phase);
	} else {
		/* assemble the frame on GPU 0 (RCCL over xGMI; the shares are disjoint) */
		crh_ctx *ctxs[MAX_GPUS];
		float *fbs[MAX_GPUS];
		for (int g = 0; g < gpus; ++g) { ctxs[g] = workers[g].ctx; fbs[g] = workers[g].fb; }
		assembleFrame(ctxs, fbs, gpus, W, H);
		gatherUs = getUs(phase);
		startTimer(&phase);
		/* 8-bit output exactly like renderer.c:294-300 — on the device — and the float buffer: one download each */
		if (crh_framebuffer_to_srgb8(workers[0].ctx, workers[0].fb, W, H, output->data.byte_p) != CRH_OK)
			logr(error, "c-ray-hip: sRGB conversion failed: %s\n", crh_last_error());
		resolveUs = getUs(phase);
		startTimer(&phase);
		if (crh_framebuffer_download(workers[0].ctx, workers[0].fb, W, H, buf->data.float_p) != CRH_OK)
			logr(error, "c-ray-hip: framebuffer download failed: %s\n", crh_last_error());
		downloadUs = getUs(phase);
	}
	const long workUs = getUs(frame);            /* set-up + dispatches + gather + conversion + downloads */
	const char *dump = getenv("CRH_DUMP_F32");
	if (dump) {
		FILE *f = fopen(dump, "wb");
		if (f) { fwrite(buf->data.float_p, sizeof(float), (size_t)W * H * 3, f); fclose(f); }
	}
	logr(info, "%llu rays traced on %i GPU%s.\n", (unsigned long long)rays, gpus, PLURAL(gpus));
	crh_adaptive_params adaptive;
	const int adapt = adaptiveSettings(r, &adaptive);
	if (getenv("CRAY_HIP_ADAPTIVE") && *getenv("CRAY_HIP_ADAPTIVE") && !adapt)
		logr(warning, "c-ray-hip: CRAY_HIP_ADAPTIVE needs a threshold >= 0, an even CRAY_HIP_ADAPTIVE_MIN >= 2 (default 16) and a sample count of that times a power of two; "
			"%i samples rendered uniformly\n", r->prefs.sampleCount);
	if (adapt && adaptiveCellSettings(NULL, NULL) < 0)
		logr(warning, "c-ray-hip: CRAY_HIP_ADAPTIVE_CELL needs an integer in 1 .. 1024; deciding per rectangle\n");
	if (adapt && !failed) {
		/* the rays spent and where: the share of the rectangles (with CRAY_HIP_ADAPTIVE_CELL: of their cells) that stopped at each pass count */
		char line[512];
		int at = 0;
		uint32_t all = 0;
		int cell = 0;
		for (int g = 0; g < gpus; ++g) { all += workers[g].adaptUnits; if (workers[g].adaptCell) cell = workers[g].adaptCell; }
		for (long n = adaptive.min_passes; n <= r->prefs.sampleCount; n *= 2) {
			uint32_t k = 0;
			for (int g = 0; g < gpus; ++g) for (uint32_t i = 0; i < workers[g].adaptUnits; ++i) k += workers[g].adaptPasses[i] == n;
			if (at < (int)sizeof(line) - 32) at += snprintf(line + at, sizeof(line) - (size_t)at, "%s%ld: %.1f %%", at ? ", " : "", n, all ? 100.0 * k / all : 0.0);
		}
		if (cell)
			logr(info, "Adaptive sampling (threshold %g, at least %i passes, cells of %i, dilate %i): %llu rays, %u cells by pass count: %s.\n", (double)adaptive.threshold,
				adaptive.min_passes, cell, (int)!(getenv("CRAY_HIP_ADAPTIVE_DILATE") && !strcmp(getenv("CRAY_HIP_ADAPTIVE_DILATE"), "0")), (unsigned long long)rays, all, line);
		else
			logr(info, "Adaptive sampling (threshold %g, at least %i passes): %llu rays, %u tiles by pass count: %s.\n", (double)adaptive.threshold, adaptive.min_passes, (unsigned long long)rays, all, line);
	}
	float *keptAov = NULL, *keptDenoised = NULL;          /* CRAY_HIP_EXR: the guides and the denoised frame stay on GPU 0 for the layers file */
	if (!workers[0].failed && !r->state.renderAborted) writeAovs(r, workers[0].ctx, W, H, layers && !failed ? &keptAov : NULL);
	if (!failed && !r->state.renderAborted) {          /* (a frame assembled on the host is not on GPU 0) */
		const int halfAt = varianceHalfPasses(r);          /* (sampleCount / 2 also describes an adaptive frame: every rectangle's half holds the first half of its passes, scale 1) */
		if (halfAt && gpus > 1) {          /* the half-sample frame: the same strips, the same way to GPU 0 */
			crh_ctx *ctxs[MAX_GPUS];
			float *halves[MAX_GPUS];
			for (int g = 0; g < gpus; ++g) { ctxs[g] = workers[g].ctx; halves[g] = workers[g].half; }
			assembleFrame(ctxs, halves, gpus, W, H);
		}
		writeDenoised(r, workers[0].ctx, workers[0].fb, halfAt ? workers[0].half : NULL, halfAt, W, H, layers ? &keptDenoised : NULL);
		if (layers) writeLayers(r, workers[0].ctx, workers[0].fb, keptAov, keptDenoised, &layerNames, W, H);
		if (gpuPng) writeGpuPng(r, workers[0].ctx, workers[0].fb, W, H);
	} else {
		if (layers) logr(warning, "c-ray-hip: CRAY_HIP_EXR needs the frame on GPU 0; no layers file\n");
		if (gpuPng) logr(warning, "c-ray-hip: CRAY_HIP_PNG needs the frame on GPU 0; no GPU PNG\n");
	}
	if (keptAov) crh_aov_free(workers[0].ctx, keptAov);
	if (keptDenoised) crh_framebuffer_free(workers[0].ctx, keptDenoised);
	layerNamesFree(&layerNames);
	if (!layers && getenv("CRAY_HIP_IDS") && atoi(getenv("CRAY_HIP_IDS")) > 0) logr(warning, "c-ray-hip: CRAY_HIP_IDS has no output without CRAY_HIP_EXR=1\n");
	if (getenv("CRAY_HIP_DESPECKLE") && !(getenv("CRAY_HIP_DENOISE") && atoi(getenv("CRAY_HIP_DENOISE")) > 0))
		logr(warning, "c-ray-hip: CRAY_HIP_DESPECKLE filters the denoiser's input and has no effect without CRAY_HIP_DENOISE\n");

	for (int g = 0; g < gpus; ++g) {
		if (workers[g].ctx && workers[g].fb) crh_framebuffer_free(workers[g].ctx, workers[g].fb);
		if (workers[g].ctx && workers[g].half) crh_framebuffer_free(workers[g].ctx, workers[g].half);
		free(workers[g].adaptTiles);
		free(workers[g].adaptPasses);
		poolRelease(g, workers[g].ctx, !workers[g].failed);
	}
	pthread_mutex_destroy(&sync.mu);
	pthread_cond_destroy(&sync.cv);
	crh_flatten_free(&scene);
	crh_compiled_scene_free(compiled);
	const long frameUs = getUs(frame);          /* the whole of renderFrame(), teardown included: what the timer of c-ray.c:279-281 sees */
	/* CRH_DUMP_STATS=<path>: where the frame went, for bench.py's `dropin` object. render_phase_ms is SURVEY.md 8(d)'s phase — the timer
	 * of src/c-ray.c:279-281 around renderFrame() minus the set-up (flatten / context / upload: everything before the slowest GPU was ready
	 * to dispatch): dispatches + gather + 8-bit conversion + downloads + the host in between. */
	const char *statsPath = getenv("CRH_DUMP_STATS");
	if (statsPath) {
		long contextUs = 0, uploadUs = 0, renderUs = 0, launchUs = 0, readyUs = 0;
		double kernelMs = 0.0;
		int dispatches = 0;
		for (int g = 0; g < gpus; ++g) {
			if (workers[g].contextUs > contextUs) contextUs = workers[g].contextUs;
			if (workers[g].uploadUs > uploadUs) uploadUs = workers[g].uploadUs;
			if (workers[g].readyUs > readyUs) readyUs = workers[g].readyUs;
			if (workers[g].renderUs > renderUs) renderUs = workers[g].renderUs;
			if (workers[g].launchUs > launchUs) launchUs = workers[g].launchUs;
			if (workers[g].kernelMs > kernelMs) kernelMs = workers[g].kernelMs;
			if (workers[g].dispatches > dispatches) dispatches = workers[g].dispatches;
		}
		FILE *f = fopen(statsPath, "w");
		if (f) {
			fprintf(f, "{\"gpus\": %d, \"width\": %d, \"height\": %d, \"samples\": %d, \"bounces\": %d, \"rays\": %llu, \"flatten_ms\": %.3f, \"compile_once_ms\": %.3f, "
					"\"context_ms\": %.3f, \"upload_ms\": %.3f, \"context_upload_ms\": %.3f, \"setup_ms\": %.3f, \"render_ms\": %.3f, \"kernel_ms\": %.3f, \"launch_host_ms\": %.3f, "
					"\"dispatches\": %d, \"reduce_download_ms\": %.3f, \"gather_ms\": %.3f, \"resolve_srgb_ms\": %.3f, \"download_ms\": %.3f, \"rccl_setup_ms\": %.3f, "
					"\"frame_ms\": %.3f, \"teardown_ms\": %.3f, \"render_phase_ms\": %.3f}\n",
					gpus, W, H, r->prefs.sampleCount, r->prefs.bounces, (unsigned long long)rays, flattenUs / 1e3, compileUs / 1e3, contextUs / 1e3, uploadUs / 1e3,
					(contextUs + uploadUs) / 1e3, readyUs / 1e3, renderUs / 1e3, kernelMs, launchUs / 1e3, dispatches, (gatherUs + downloadUs) / 1e3, gatherUs / 1e3,
					resolveUs / 1e3, downloadUs / 1e3, warm.us / 1e3, frameUs / 1e3, (frameUs - workUs) / 1e3, (workUs - readyUs) / 1e3);
			fclose(f);
		}
	}

	return output;
}

struct renderer *newRenderer(void) {
	struct renderer *r = calloc(1, sizeof(*r));
	/* the estimators in ui.c / renderer statistics divide by these, so they start at 1 (renderer.c:331-333) */
	r->state.timeSampleCount = 1;
	r->state.finishedPasses = 1;
	r->state.avgTileTime = 1;
	r->state.tileMutex = createMutex();
	r->state.timer = calloc(1, sizeof(*r->state.timer));
	if (!g_vertices) allocVertexBuffers();
	if (!isSet("is_worker")) poolPrefetch();          /* (a cluster worker makes its own context when its first tile arrives: host/access/worker_access.c) */
	return r;
}

void destroyRenderer(struct renderer *r) {
	if (!r) return;
	poolDestroy();
	destroyScene(r->scene);
	destroyTexture(r->state.uiBuffer);
	destroyTexture(r->state.renderBuffer);
	destroyVertexBuffers();
	free(r->state.threadStates);
	free(r->state.threads);
	free(r->state.renderTiles);
	free(r->state.tileMutex);
	free(r->state.timer);
	free(r->prefs.assetPath);
	free(r->prefs.imgFilePath);
	free(r->prefs.imgFileName);
	free(r);
}
