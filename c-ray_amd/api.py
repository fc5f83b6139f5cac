"""api.py — thin ctypes binding of libcray_hip.so (include/cray_hip.h).

Plumbing, not the product: everything that computes lives behind the C-ABI in c-ray_amd/csrc. There is
no CPU fallback here either: `library()` raises if the HIP library has not been built, and every call
raises `CrhError` on a non-zero return code (the reference's convention is 0 = ok, negative = failure,
src/datatypes/scene.c:122-134).
"""
import ctypes as C
import os

import numpy as np

from . import abi, exr

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CRH_LIB") or os.path.join(HERE, "_lib", "libcray_hip.so")    # CRH_LIB: A/B another build (dev)


class CrhError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__(f"{where} failed with {code}: {detail}")


_lib = None


def library():
    """Load libcray_hip.so (built by c-ray_amd/build.py). Raises loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} is missing: run `python c-ray_amd/build.py` "
                                "(or __graft_entry__.build()); there is no CPU fallback")
    # torch wheels bundle their own libamdhip64; whichever HIP runtime is loaded first owns the device, and a second copy
    # then reports "No HIP GPUs". Let torch (when present) load its copy first: libcray_hip's NEEDED libamdhip64 resolves to it.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    # The emulation library of tests/emu — the kernels compiled for the CPU on a HIP shim — exports the same C-ABI. It is test infrastructure: only
    # a caller that says so explicitly (the emulation tier's child processes and the tools/emu_* scripts) may bind to it.
    if hasattr(L, "crh_emu_stats") and os.environ.get("CRH_ALLOW_EMULATION") != "1":
        raise RuntimeError(f"{LIB_PATH} is the CPU emulation of the kernels (test infrastructure): the product has no CPU path "
                           "(set CRH_ALLOW_EMULATION=1 only in tests / tools that mean it)")
    ctx = C.c_void_p
    sig = {
        "crh_device_count": (C.c_int, []),
        "crh_last_error": (C.c_char_p, []),
        "crh_abi_version": (C.c_int, []),
        "crh_context_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(ctx)]),
        "crh_context_destroy": (C.c_int, [ctx]),
        "crh_set_option": (C.c_int, [ctx, C.c_int, C.c_int64]),
        "crh_debug_wave_stats": (C.c_int, [ctx, C.c_void_p, C.c_uint32]),
        "crh_debug_phase_ticks": (C.c_int, [ctx, C.c_void_p]),
        "crh_scene_upload": (C.c_int, [ctx, C.POINTER(abi.SceneDesc)]),
        "crh_scene_compile": (C.c_int, [C.POINTER(abi.SceneDesc), C.c_int, C.POINTER(C.c_void_p)]),
        "crh_scene_upload_compiled": (C.c_int, [ctx, C.c_void_p]),
        "crh_compiled_scene_free": (None, [C.c_void_p]),
        "crh_debug_upload_counts": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "crh_framebuffer_alloc": (C.c_int, [ctx, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
        "crh_framebuffer_free": (C.c_int, [ctx, C.c_void_p]),
        "crh_framebuffer_clear": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int]),
        "crh_framebuffer_download": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
        "crh_framebuffer_to_srgb8": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
        "crh_framebuffer_strips_to_srgb8": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
        "crh_render_region": (C.c_int, [ctx, C.POINTER(abi.RenderParams), C.c_void_p]),
        "crh_render_tiles": (C.c_int, [ctx, C.POINTER(abi.RenderParams), C.POINTER(abi.Tile), C.c_uint32, C.c_void_p]),
        "crh_aov_alloc": (C.c_int, [ctx, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
        "crh_aov_free": (C.c_int, [ctx, C.c_void_p]),
        "crh_aov_clear": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int]),
        "crh_aov_download": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
        "crh_render_aov": (C.c_int, [ctx, C.POINTER(abi.RenderParams), C.POINTER(abi.Tile), C.c_uint32, C.c_void_p]),
        "crh_aov_kernel_time_ms": (C.c_int, [ctx, C.POINTER(C.c_float)]),
        "crh_ids_alloc": (C.c_int, [ctx, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
        "crh_ids_free": (C.c_int, [ctx, C.c_void_p]),
        "crh_ids_clear": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int]),
        "crh_ids_download": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
        "crh_render_ids": (C.c_int, [ctx, C.POINTER(abi.RenderParams), C.POINTER(abi.Tile), C.c_uint32, C.c_void_p, C.c_void_p]),
        "crh_ids_kernel_time_ms": (C.c_int, [ctx, C.POINTER(C.c_float)]),
        "crh_ids_resolve": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
        "crh_ids_matte": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.c_void_p]),
        "crh_pack_scanlines": (C.c_int, [ctx, C.POINTER(abi.PackChannel), C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
        "crh_pack_time_ms": (C.c_int, [ctx, C.POINTER(C.c_float)]),
        "crh_denoise_params_default": (None, [C.POINTER(abi.DenoiseParams)]),
        "crh_denoise": (C.c_int, [ctx, C.POINTER(abi.DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p]),
        "crh_denoise_time_ms": (C.c_int, [ctx, C.POINTER(C.c_float)]),
        "crh_debug_denoise_launch_ms": (C.c_int, [ctx, C.POINTER(C.c_float), C.c_uint32]),
        "crh_denoise_variance_params_default": (None, [C.POINTER(abi.DenoiseVarianceParams), C.c_int, C.c_int]),
        "crh_denoise_variance": (C.c_int, [ctx, C.POINTER(abi.DenoiseVarianceParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "crh_framebuffer_copy": (C.c_int, [ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
        "crh_adaptive_step": (C.c_int, [ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(abi.Tile), C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]),
        "crh_adaptive_time_ms": (C.c_int, [ctx, C.POINTER(C.c_float)]),
        "crh_adaptive_params_default": (None, [C.POINTER(abi.AdaptiveParams)]),
        "crh_render_adaptive": (C.c_int, [ctx, C.POINTER(abi.RenderParams), C.POINTER(abi.Tile), C.c_uint32, C.POINTER(abi.AdaptiveParams), C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
        "crh_adaptive_cell_offsets": (C.c_int64, [C.POINTER(abi.Tile), C.c_uint32, C.c_int, C.c_void_p]),
        "crh_adaptive_step_cells": (C.c_int, [ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(abi.Tile), C.c_uint32, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
        "crh_adaptive_cells_params_default": (None, [C.POINTER(abi.AdaptiveCellsParams)]),
        "crh_render_adaptive_cells": (C.c_int, [ctx, C.POINTER(abi.RenderParams), C.POINTER(abi.Tile), C.c_uint32, C.POINTER(abi.AdaptiveCellsParams), C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
        "crh_synchronize": (C.c_int, [ctx]),
        "crh_frames_reduce": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]),
        "crh_frames_gather": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]),
        "crh_frames_prepare": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
        "crh_context_prepare": (C.c_int, [ctx]),
        "crh_counters_get": (C.c_int, [ctx, C.POINTER(abi.Counters)]),
        "crh_counters_reset": (C.c_int, [ctx]),
        "crh_kernel_time_ms": (C.c_int, [ctx, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "crh_last_kernel_name": (C.c_char_p, [ctx]),
        "crh_trace_rays": (C.c_int, [ctx, C.c_void_p, C.c_uint64, C.c_void_p]),
        "crh_debug_eval_math": (C.c_int, [ctx, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
        "crh_bvh_build_triangles": (C.c_int, [ctx, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_uint32), C.POINTER(abi.BvhBuildStats)]),
        "crh_blob_save": (C.c_int, [C.c_char_p, C.POINTER(abi.SceneDesc), C.POINTER(abi.BlobPrefs)]),
        "crh_blob_load": (C.c_int, [C.c_char_p, C.POINTER(C.POINTER(abi.SceneDesc)), C.POINTER(abi.BlobPrefs)]),
        "crh_blob_free": (None, [C.POINTER(abi.SceneDesc)]),
        "crh_debug_ray_dump": (C.c_int, [ctx, C.c_uint32]),
        "crh_debug_ray_dump_counts": (C.c_int, [ctx, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint32]),
        "crh_debug_ray_dump_fetch": (C.c_int, [ctx, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
        "crh_debug_walk_probe": (C.c_int, [ctx, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]),
        "crh_debug_walk_probe_fetch": (C.c_int, [ctx, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
        "crh_debug_walk_probe_compare": (C.c_int, [ctx, C.POINTER(C.c_uint64)]),
        "crh_debug_plan_units": (C.c_int, [C.POINTER(abi.RenderParams), C.POINTER(abi.Tile), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _check(rc, where):
    if rc != 0:
        raise CrhError(rc, where, (library().crh_last_error() or b"").decode(errors="replace"))


def _tile_array(tiles):
    """A list of (x0, y0, x1, y1) as the C entries take it: a crh_tile array, NULL for an empty list (every entry accepts NULL beside a count of 0)."""
    n = len(tiles)
    return (abi.Tile * n)(*[abi.Tile(*t) for t in tiles]) if n else None


def device_count():
    return library().crh_device_count()


def sample_count_map(width, height, tiles, passes):
    """What a compositor asks of an adaptive frame: the int32 [height, width] map of samples per pixel in stored order (row 0 = the top of the image) from
    Context.render_adaptive's per-tile pass counts; 0 where no tile lies."""
    out = np.zeros((height, width), np.int32)
    for (x0, y0, x1, y1), n in zip(tiles, passes):
        out[height - y1:height - y0, x0:x1] = n
    return out


def adaptive_cell_offsets(tiles, cell):
    """crh_adaptive_cell_offsets: the uint32 [n + 1] index of every rectangle's first cell in the cell-granular arrays (the last entry is the total): a rectangle
    of tw x th pixels holds ceil(tw / cell) x ceil(th / cell) cells, rows of cells from its first stored row down, x ascending within a row."""
    n = len(tiles)
    arr = _tile_array(tiles)
    out = np.zeros(n + 1, np.uint32)
    total = library().crh_adaptive_cell_offsets(arr, n, cell, out.ctypes.data)
    if total < 0:
        _check(int(total), "crh_adaptive_cell_offsets")
    return out


def sample_count_map_cells(width, height, tiles, cell, cell_passes):
    """sample_count_map for Context.render_adaptive_cells' per-cell pass counts: the int32 [height, width] map, 0 where no rectangle lies."""
    out = np.zeros((height, width), np.int32)
    offsets = adaptive_cell_offsets(tiles, cell)
    for (x0, y0, x1, y1), first in zip(tiles, offsets):
        cx, cy = -(-(x1 - x0) // cell), -(-(y1 - y0) // cell)
        counts = np.asarray(cell_passes[int(first):int(first) + cx * cy], np.int32).reshape(cy, cx)
        out[height - y1:height - y0, x0:x1] = np.repeat(np.repeat(counts, cell, 0), cell, 1)[:y1 - y0, :x1 - x0]
    return out


class CompiledScene:
    """crh_scene_compile: the device layout of a scene, derived once on the host; any number of contexts upload it (Context.upload_compiled)."""

    def __init__(self, scene, walk=0):
        desc = scene.ptr if hasattr(scene, "ptr") else C.pointer(scene)
        self.h = C.c_void_p()
        _check(library().crh_scene_compile(desc, walk, C.byref(self.h)), "crh_scene_compile")

    def close(self):
        if self.h:
            library().crh_compiled_scene_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def upload_counts():
    """(layout compiles, uploads) of this process so far (crh_debug_upload_counts)."""
    a, b = C.c_int(0), C.c_int(0)
    library().crh_debug_upload_counts(C.byref(a), C.byref(b))
    return a.value, b.value


def plan_units(width, height, samples, tiles, cu_count=256, first_pass=0, pass_count=None):
    """crh_debug_plan_units (no device needed): the work units of one dispatch in hand-out order, as an int32 array [n, 8] of
    x0, y0, x1, y1, block area, taper level, first pass, pass count — and the pass chunk."""
    p = abi.RenderParams(0, 0, 0, 0, width, height, first_pass, samples - first_pass if pass_count is None else pass_count, samples, 1)
    arr = _tile_array(tiles)
    n, chunk = C.c_uint64(0), C.c_int32(0)
    _check(library().crh_debug_plan_units(C.byref(p), arr, len(tiles), cu_count, None, 0, C.byref(n), C.byref(chunk)), "crh_debug_plan_units")
    units = np.zeros((n.value, 8), np.int32)
    _check(library().crh_debug_plan_units(C.byref(p), arr, len(tiles), cu_count, units.ctypes.data, n.value, C.byref(n), C.byref(chunk)), "crh_debug_plan_units")
    return units, chunk.value


class Scene:
    """A flat scene blob (written by the flattener, c-ray_amd/host/flatten.c) loaded through the library."""

    def __init__(self, path):
        self.path = path
        self.ptr = C.POINTER(abi.SceneDesc)()
        self.prefs = abi.BlobPrefs()
        rc = library().crh_blob_load(os.fsencode(path), C.byref(self.ptr), C.byref(self.prefs))
        if rc != 0:
            raise CrhError(rc, f"crh_blob_load({path})")

    @property
    def desc(self):
        return self.ptr.contents

    def close(self):
        if self.ptr:
            library().crh_blob_free(self.ptr)
            self.ptr = C.POINTER(abi.SceneDesc)()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One crh_ctx = one GPU. `stream` may be a raw hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)."""

    def __init__(self, device=0, stream=None):
        self.L = library()
        self.h = C.c_void_p()
        _check(self.L.crh_context_create(int(device), C.c_void_p(stream) if stream else None, C.byref(self.h)),
               "crh_context_create")
        self._owned_fbs = []
        self._owned_aovs = []
        self._owned_ids = []
        self._device, self._stream, self._zip = int(device), stream, None

    def _zip_context(self):
        """The companion library's context of write_layers_exr(compression=...): on this context's device, on the caller's stream if one was given; made on first use."""
        if self._zip is None:
            from . import exrzip
            self._zip = exrzip.ZipContext(self._device, self._stream)
        return self._zip

    def close(self):
        if getattr(self, "_zip", None) is not None:
            self._zip.close()
            self._zip = None
        if self.h:
            for fb in self._owned_fbs:
                self.L.crh_framebuffer_free(self.h, fb)
            self._owned_fbs = []
            for buf in self._owned_aovs:
                self.L.crh_aov_free(self.h, buf)
            self._owned_aovs = []
            for buf in self._owned_ids:
                self.L.crh_ids_free(self.h, buf)
            self._owned_ids = []
            self.L.crh_context_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, option, value):
        _check(self.L.crh_set_option(self.h, int(option), int(value)), "crh_set_option")

    def wave_stats(self):
        buf = np.zeros((8192, 2), dtype=np.uint64)
        n = self.L.crh_debug_wave_stats(self.h, buf.ctypes.data, 8192)
        if n < 0:
            _check(n, "crh_debug_wave_stats")
        return buf[:n]

    def phase_ticks(self):
        buf = np.zeros(24, dtype=np.uint64)
        _check(self.L.crh_debug_phase_ticks(self.h, buf.ctypes.data), "crh_debug_phase_ticks")
        keys = ("setup", "traverse", "shade", "w_node", "w_tri", "w_ctrl", "w_round", "w_shade", "w_setup", "u_node", "u_shade",
                "t_swap", "t_gen", "n_swap", "n_gen", "u_swap", "u_tri", "u_ctrl", "w_tri_in", "u_tri_in", "w_ctrl_in", "u_ctrl_in", "u_wait_tri", "u_wait_fin")
        return {k: int(v) for k, v in zip(keys, buf)}

    def prepare(self):
        """crh_context_prepare: per-wave buffers + code objects before the scene is there (optional)."""
        _check(self.L.crh_context_prepare(self.h), "crh_context_prepare")

    def set_sched(self, node, tri, ctrl, swap_min, fill_to=160, run_num=4, tri_in_run=12, ctrl_in_run=12, shade_min=0, swap_in_run=20):
        """shade_min = 0 keeps the library's tuned value (include/cray_hip.h: CRH_OPT_SCHED_RUNS)."""
        self.set_option(abi.OPT_SCHED_WEIGHTS, node | (tri << 12) | (ctrl << 24) | (swap_min << 36))
        self.set_option(abi.OPT_SCHED_RUNS, fill_to | (run_num << 12) | (tri_in_run << 16) | (ctrl_in_run << 24) | (shade_min << 32) | (swap_in_run << 40))

    def set_sched_wg(self, linger=8, drain_at=192, max_drainers=1, partial_min=16, walk_min=32, fill_to=768):
        """Scheduler of the workgroup kernel (CRH_OPT_KERNEL = KERNEL_WG), see cray_hip.hip: k_pathtrace_wg."""
        self.set_option(abi.OPT_SCHED_WG, linger | (drain_at << 8) | (max_drainers << 20) | (partial_min << 24) | (walk_min << 32) | (fill_to << 40))

    def upload(self, scene):
        desc = scene.ptr if hasattr(scene, "ptr") else C.pointer(scene)
        _check(self.L.crh_scene_upload(self.h, desc), "crh_scene_upload")

    def upload_compiled(self, compiled):
        """crh_scene_upload_compiled: the copies only, from a CompiledScene (one layout compile for several contexts)."""
        _check(self.L.crh_scene_upload_compiled(self.h, compiled.h), "crh_scene_upload_compiled")

    def framebuffer(self, width, height):
        p = C.c_void_p()
        _check(self.L.crh_framebuffer_alloc(self.h, width, height, C.byref(p)), "crh_framebuffer_alloc")
        self._owned_fbs.append(p)
        return p

    def clear(self, fb, width, height):
        _check(self.L.crh_framebuffer_clear(self.h, fb, width, height), "crh_framebuffer_clear")

    def render_region(self, fb, width, height, samples, bounces, region=None, first_pass=0, pass_count=None):
        x0, y0, x1, y1 = region if region else (0, 0, width, height)
        p = abi.RenderParams(x0, y0, x1, y1, width, height, first_pass,
                             samples - first_pass if pass_count is None else pass_count, samples, bounces)
        _check(self.L.crh_render_region(self.h, C.byref(p), fb), "crh_render_region")

    def render_tiles(self, fb, width, height, samples, bounces, tiles, first_pass=0, pass_count=None):
        p = abi.RenderParams(0, 0, 0, 0, width, height, first_pass,
                             samples - first_pass if pass_count is None else pass_count, samples, bounces)
        arr = _tile_array(tiles)
        _check(self.L.crh_render_tiles(self.h, C.byref(p), arr, len(tiles), fb), "crh_render_tiles")

    # ---- AOV buffers: albedo, normal, depth, coverage of every camera ray's first hit (include/cray_hip.h: crh_render_aov) ----
    def aov_buffer(self, width, height):
        """A zeroed device buffer of abi.AOV_CHANNELS floats per pixel, owned by the context."""
        p = C.c_void_p()
        _check(self.L.crh_aov_alloc(self.h, width, height, C.byref(p)), "crh_aov_alloc")
        self._owned_aovs.append(p)
        return p

    def clear_aov(self, buf, width, height):
        _check(self.L.crh_aov_clear(self.h, buf, width, height), "crh_aov_clear")

    def render_aov(self, buf, width, height, samples, tiles=None, region=None, first_pass=0, pass_count=None):
        """Fold passes [first_pass, first_pass + pass_count) of `samples` into `buf`: the pixels of `tiles` (a list of x0, y0, x1, y1), or of `region`, or the whole image."""
        x0, y0, x1, y1 = region if region else (0, 0, width, height)
        p = abi.RenderParams(x0, y0, x1, y1, width, height, first_pass, samples - first_pass if pass_count is None else pass_count, samples, 0)
        if tiles is None:
            _check(self.L.crh_render_aov(self.h, C.byref(p), None, 0, buf), "crh_render_aov")
        elif len(tiles):          # (an empty list is no work; to the C entry a count of 0 means "the region of params")
            arr = _tile_array(tiles)
            _check(self.L.crh_render_aov(self.h, C.byref(p), arr, len(tiles), buf), "crh_render_aov")

    def download_aov(self, buf, width, height):
        """float32 [height, width, 8]: albedo r g b, normal x y z, depth, coverage (row 0 = the top of the image, like download())."""
        out = np.empty((height, width, abi.AOV_CHANNELS), dtype=np.float32)
        _check(self.L.crh_aov_download(self.h, buf, width, height, out.ctypes.data), "crh_aov_download")
        return out

    def aov_kernel_time_ms(self):
        """Milliseconds of the most recent render_aov's kernel (waits for it)."""
        ms = C.c_float(0.0)
        _check(self.L.crh_aov_kernel_time_ms(self.h, C.byref(ms)), "crh_aov_kernel_time_ms")
        return float(ms.value)

    # ---- ID mattes: ranked instance and material coverage per pixel (include/cray_hip.h: crh_render_ids) ----
    def ids_buffer(self, width, height):
        """A zeroed device buffer of abi.ID_WORDS uint32 per pixel, owned by the context."""
        p = C.c_void_p()
        _check(self.L.crh_ids_alloc(self.h, width, height, C.byref(p)), "crh_ids_alloc")
        self._owned_ids.append(p)
        return p

    def clear_ids(self, buf, width, height):
        _check(self.L.crh_ids_clear(self.h, buf, width, height), "crh_ids_clear")

    def render_ids(self, instance_ids, material_ids, width, height, samples, tiles=None, region=None, first_pass=0, pass_count=None):
        """Fold the first hits of passes [first_pass, first_pass + pass_count) of `samples` into the instance-id buffer and the material-id buffer (either may be None):
        the pixels of `tiles` (a list of x0, y0, x1, y1), or of `region`, or the whole image."""
        x0, y0, x1, y1 = region if region else (0, 0, width, height)
        p = abi.RenderParams(x0, y0, x1, y1, width, height, first_pass, samples - first_pass if pass_count is None else pass_count, samples, 0)
        if tiles is None:
            _check(self.L.crh_render_ids(self.h, C.byref(p), None, 0, instance_ids, material_ids), "crh_render_ids")
        elif len(tiles):          # (an empty list is no work; to the C entry a count of 0 means "the region of params")
            arr = _tile_array(tiles)
            _check(self.L.crh_render_ids(self.h, C.byref(p), arr, len(tiles), instance_ids, material_ids), "crh_render_ids")

    def download_ids(self, buf, width, height):
        """uint32 [height, width, 16]: id[0..5], count[0..5], lost, total, two reserved words (row 0 = the top of the image, like download())."""
        out = np.empty((height, width, abi.ID_WORDS), dtype=np.uint32)
        _check(self.L.crh_ids_download(self.h, buf, width, height, out.ctypes.data), "crh_ids_download")
        return out

    def resolve_ids(self, buf, width, height, out):
        """Rank the slots of every pixel of `buf` by coverage into the device float buffer `out` [height, width, 6, 2]: (id, coverage) pairs, an empty rank (-1, 0)."""
        _check(self.L.crh_ids_resolve(self.h, buf, width, height, out), "crh_ids_resolve")

    def ids_matte(self, buf, width, height, ids, out):
        """The coverage of the ids of the list `ids` in every pixel of `buf` into the device float buffer `out` [height, width]."""
        ids = [int(i) for i in ids]
        arr = (C.c_uint32 * len(ids))(*ids) if ids else None
        _check(self.L.crh_ids_matte(self.h, buf, width, height, arr, len(ids), out), "crh_ids_matte")

    def ids_kernel_time_ms(self):
        """Milliseconds of the most recent ID kernel — render_ids', resolve_ids' or ids_matte's (waits for it)."""
        ms = C.c_float(0.0)
        _check(self.L.crh_ids_kernel_time_ms(self.h, C.byref(ms)), "crh_ids_kernel_time_ms")
        return float(ms.value)

    # ---- the multi-layer OpenEXR output (include/cray_hip.h: crh_pack_scanlines; the file around the pixel data: exr.py) ----
    def pack_scanlines(self, channels, width, height, first_row=0, row_count=None):
        """The pixel data of stored rows [first_row, first_row + row_count) (None: to the last row) as bytes: per row int32 y, int32 4 * channels * width and one plane
        of `width` 32-bit words per channel, in the order given. A channel is (device pointer, stride, component) or (device pointer, stride, component, map): a
        component of a float buffer [height, width, stride]; with a map — a uint32 array — the value is an id and the word is map[id], 0 for anything that is not
        an id below len(map)."""
        n = len(channels)
        arr, keep = abi.pack_channels(channels)
        rows = height - first_row if row_count is None else row_count
        out = np.empty(max(rows, 0) * (2 + n * width), np.uint32)
        _check(self.L.crh_pack_scanlines(self.h, arr, n, width, height, first_row, rows, out.ctypes.data), "crh_pack_scanlines")
        del keep          # (the maps' arrays lived until the call returned)
        return out.tobytes()

    def pack_time_ms(self):
        """Milliseconds of the most recent pack_scanlines' kernel (waits for it)."""
        ms = C.c_float(0.0)
        _check(self.L.crh_pack_time_ms(self.h, C.byref(ms)), "crh_pack_time_ms")
        return float(ms.value)

    def write_layers_exr(self, path, width, height, fb, aov=None, denoised=None, instance_ids=None, material_ids=None, instance_names=None, material_names=None,
                         chunk_rows=None, compression="none", half=False, codes="fixed"):
        """One multi-layer OpenEXR file (scanline, FLOAT channels; HALF ones with `half`) of the frame `fb` and whichever of the others is given: R G B; the guides of
        an AOV buffer as albedo.R/G/B, normal.X/Y/Z, Z and A, unscaled; a denoised frame as denoised.R/G/B; the ID buffers `instance_ids` / `material_ids`
        (render_ids) as the Cryptomatte layers CryptoObject00..02 / CryptoMaterial00..02 with their metadata. instance_names[i] / material_names[i] name id i
        (default instance#<i> / material#<i>, for every id up to the largest one the buffer holds). The ranking runs into scratch of this call's own; the pixel data is
        packed on the device, `chunk_rows` rows at a time (None: all at once). compression: "none", or "zips" / "zip" — a chunk a row / every 16 rows, deflated on the
        device by the companion library (exrzip.py: loaded on first use; `chunk_rows` is rounded up to a multiple of 16 for "zip").
        half: True stores the colour layers that are present — R G B, albedo.R/G/B, normal.X/Y/Z, denoised.R/G/B — as 16-bit HALF channels, as compositors expect
        them; Z, A and the Cryptomatte channels stay FLOAT. An iterable of channel names stores exactly those as HALF; a name the file does not have, or a
        Cryptomatte channel, raises ValueError. The conversion rounds to nearest even (include/cray_hip_exr.h); values above 65504 become infinity — that is
        the format, not a fault. Only the uncompressed all-FLOAT file is packed by this library alone (crh_pack_scanlines) and can be written where the companion
        library is not built; every other one by crx_pack.
        codes: "fixed" — the default, the deflate blocks there have always been — or "dynamic": every 4 096-byte segment of a "zip" / "zips" chunk is coded with the
        cheaper of the fixed Huffman codes and a dynamic code built on the device from its own counts (crx_set_codes: set on the companion context for this call,
        then put back to what it was). The pixels are the same, the file is never larger; with compression "none" the argument has no effect. Another value
        raises ValueError."""
        from . import exrzip          # (binds the companion library on first use)
        if compression not in exrzip.COMPRESSION:
            raise ValueError(f"compression {compression!r}: one of {sorted(exrzip.COMPRESSION)}")
        if codes not in exrzip.CODES:
            raise ValueError(f"codes {codes!r}: one of {sorted(exrzip.CODES)}")
        ranked, maps, strings, scratch = [None, None], [None, None], {}, []
        try:
            for k, (ids, names, stem) in enumerate(((instance_ids, instance_names, "instance"), (material_ids, material_names, "material"))):
                if ids is None:
                    continue
                if names is None:
                    words = self.download_ids(ids, width, height)
                    used = words[..., abi.ID_SLOTS:2 * abi.ID_SLOTS] != 0
                    names = [f"{stem}#{i}" for i in range(int(words[..., :abi.ID_SLOTS][used].max()) + 1 if used.any() else 0)]
                names = list(names) or [f"{stem}#0"]          # (a map has at least one entry)
                p = C.c_void_p()          # [H, W, 6, 2] floats fit an ID buffer's 16 words a pixel
                _check(self.L.crh_ids_alloc(self.h, width, height, C.byref(p)), "crh_ids_alloc")
                scratch.append(p)
                self.resolve_ids(ids, width, height, p)
                ranked[k], maps[k] = p, exr.id_map(names)
                strings.update(exr.crypto_attributes(exr.CRYPTO_LAYERS[k], names))
            chans = exr.layer_channels(fb, aov, denoised, ranked[0], ranked[1], maps[0], maps[1])
            names, sources = [c[0] for c in chans], [c[1:] for c in chans]
            kind, lines = exrzip.COMPRESSION[compression]
            step = -(-(chunk_rows or height) // lines) * lines
            types = exr.half_types(names, half) if half else None
            if kind == 0 and types is None:
                data, sizes = b"".join(self.pack_scanlines(sources, width, height, y, min(step, height - y)) for y in range(0, height, step)), None
            else:
                self.synchronize()          # the companion's stream may be another: its sources must be complete
                z = self._zip_context()
                before = z.codes
                z.set_codes(codes)
                try:
                    parts = [z.pack(sources, width, height, kind, types, y, min(step, height - y)) for y in range(0, height, step)]
                finally:
                    z.set_codes(before)
                data, sizes = b"".join(p[0] for p in parts), np.concatenate([p[1] for p in parts])
        finally:
            for p in scratch:
                self.L.crh_ids_free(self.h, p)
        with open(path, "wb") as f:
            f.write(exr.file_bytes(width, height, names, data, sizes, strings, kind, types))
        return names

    def write_png(self, path, width, height, fb, filter="adaptive", codes="dynamic", text=None, exposure=1.0, tonemap="clamp", white=4.0, dither=False,
                  auto_permille=500, auto_target=0.18):
        """The 8-bit picture of the device frame `fb` — any frame of that shape, a denoised one for example — as a PNG file: the bytes of to_srgb8, filtered,
        deflated and check-summed on the device by the companion library (exrzip.py, crx_png_pack: loaded on first use). filter: "adaptive" (per row the PNG filter
        with the least sum of min(v, 256 - v)) or "none", "sub", "up", "average", "paeth" on every row. codes: "dynamic" — the default here: per 4 096-byte segment
        the cheaper of the fixed Huffman codes and a dynamic code — or "fixed"; set on the companion context for this call, then put back. text: tEXt chunks, a
        mapping or (key, value) pairs, Latin-1, keys of 1 .. 79 bytes. Returns the file's byte count. An unknown filter, codes or tonemap name raises ValueError.
        The display transform (crx_png_pack_display, include/cray_hip_exr.h), between the float and the byte: exposure — a factor, or "auto": the one
        ZipContext.auto_exposure measures on the device, which takes the auto_permille / 1000 quantile of the luminances to auto_target —; tonemap, a name of
        exrzip.CURVES ("clamp", "reinhard", "aces", "hable") with its white point; dither, the ordered 8 x 8 one. The defaults are the identity: the file of a call
        without them, byte for byte. Otherwise one more tEXt chunk, "C-ray Display", behind `text` says what was done, the exposure printed with %.9g."""
        from . import exrzip          # (binds the companion library on first use)
        if filter not in exrzip.PNG_FILTERS:
            raise ValueError(f"filter {filter!r}: one of {sorted(exrzip.PNG_FILTERS)}")
        if codes not in exrzip.CODES:
            raise ValueError(f"codes {codes!r}: one of {sorted(exrzip.CODES)}")
        if tonemap not in exrzip.CURVES:
            raise ValueError(f"tonemap {tonemap!r}: one of {sorted(exrzip.CURVES)}")
        auto = isinstance(exposure, str)
        if auto and exposure != "auto":
            raise ValueError(f'exposure {exposure!r}: a number or "auto"')
        self.synchronize()          # the companion's stream may be another: the frame must be complete
        z = self._zip_context()
        if auto:
            exposure = z.auto_exposure(fb, width, height, auto_permille, auto_target)[0]
        exposure = float(np.float32(exposure))
        display, texts = None, list(text.items()) if hasattr(text, "items") else list(text or ())
        if exposure != 1.0 or tonemap != "clamp" or dither:
            display = dict(exposure=exposure, curve=tonemap, white=white, dither=1 if dither else 0)
            how = f" (auto {int(auto_permille)}/1000 of {float(auto_target):.9g})" if auto else ""
            texts.append(("C-ray Display", f"exposure={exposure:.9g}{how} curve={tonemap} white={float(white):.9g} dither={display['dither']}"))
        before = z.codes
        z.set_codes(codes)
        try:
            data = z.png(fb, width, height, filter, texts, display)
        finally:
            z.set_codes(before)
        with open(path, "wb") as f:
            f.write(data)
        return len(data)

    # ---- the guided a-trous denoiser (include/cray_hip.h: crh_denoise) ----
    def denoise(self, fb, aov, width, height, out=None, **params):
        """Filter the float RGB frame `fb` guided by the AOV buffer `aov` into `out` (None: in place). Device pointers, the context's or the caller's;
        params: iterations, sigma_normal, sigma_depth, sigma_color (crh_denoise_params_default otherwise). Asynchronous on the context's stream."""
        p = abi.DenoiseParams()
        self.L.crh_denoise_params_default(C.byref(p))
        p.width, p.height = width, height
        for k, v in params.items():
            if k not in ("iterations", "sigma_normal", "sigma_depth", "sigma_color"):
                raise TypeError(f"denoise() got an unexpected parameter {k!r}")
            setattr(p, k, v)
        _check(self.L.crh_denoise(self.h, C.byref(p), fb, aov, fb if out is None else out), "crh_denoise")

    def denoise_variance(self, fb, half, aov, width, height, half_passes, passes, out=None, **params):
        """denoise() with the colour weight in units of each pixel's standard deviation (crh_denoise_variance): `half` is the frame after the first `half_passes`
        of its `passes` passes (copy_framebuffer between two dispatches). params: iterations, sigma_normal, sigma_depth, sigma_color, variance_scale."""
        p = abi.DenoiseVarianceParams()
        self.L.crh_denoise_variance_params_default(C.byref(p), half_passes, passes)
        p.width, p.height = width, height
        for k, v in params.items():
            if k not in ("iterations", "sigma_normal", "sigma_depth", "sigma_color", "variance_scale"):
                raise TypeError(f"denoise_variance() got an unexpected parameter {k!r}")
            setattr(p, k, v)
        _check(self.L.crh_denoise_variance(self.h, C.byref(p), fb, half, aov, fb if out is None else out), "crh_denoise_variance")

    def despeckle(self, fb, width, height, also=(), **params):
        """The firefly filter in front of a denoiser (include/cray_hip_exr.h: crx_despeckle): every pixel of `fb` brighter than factor * (the rank-th largest
        luminance among its neighbours within radius) + floor is scaled down to that limit, NaN and infinite pixels become 0. CHANGES `fb` IN PLACE — it removes
        energy: copy_framebuffer first to keep the original, and filter the copy — and scales every frame of `also` (the half-sample buffer of denoise_variance)
        by the same per-pixel plane. params: radius, rank, factor, floor (2, 4, 4, 2^-6 otherwise); an unknown name raises TypeError. Waits for this context's
        stream, runs on the companion library's context and waits for it. Returns the stats: clamped, bad, max_clamped, min_scale."""
        self.synchronize()
        return self._zip_context().despeckle(fb, width, height, (fb,) + tuple(also), **params)

    def copy_framebuffer(self, src, dst, width, height):
        """dst = src on the device, in stream order (crh_framebuffer_copy)."""
        _check(self.L.crh_framebuffer_copy(self.h, src, dst, width, height), "crh_framebuffer_copy")

    # ---- adaptive sampling at tile granularity (include/cray_hip.h: crh_adaptive_step, crh_render_adaptive) ----
    def adaptive_step(self, fb, half, width, height, tiles, threshold):
        """One step over `tiles` (a list of x0, y0, x1, y1): (errors float32 [n], flags bool [n]); where a tile's flag is set — its error is not <= threshold —
        half := fb over it. Waits for the result. threshold = inf measures only."""
        n = len(tiles)
        arr = _tile_array(tiles)
        errors, flags = np.zeros(n, np.float32), np.zeros(n, np.uint8)
        _check(self.L.crh_adaptive_step(self.h, fb, half, width, height, arr, n, threshold, errors.ctypes.data, flags.ctypes.data), "crh_adaptive_step")
        return errors, flags.astype(bool)

    def render_adaptive(self, fb, half, width, height, max_samples, bounces, tiles, min_passes=16, threshold=0.05, passes=None):
        """crh_render_adaptive: min_passes on every tile, then every tile doubles its pass count until its error is at most `threshold` or it reaches the cap
        `passes` (None: max_samples, which seeds the sampler). Returns (passes per tile int32 [n], error per tile float32 [n]); fb holds each tile's mean of its
        passes, half the mean of the first half of them."""
        n = len(tiles)
        p = abi.RenderParams(0, 0, 0, 0, width, height, 0, max_samples if passes is None else passes, max_samples, bounces)
        a = abi.AdaptiveParams(min_passes, threshold)
        arr = _tile_array(tiles)
        count, errors = np.zeros(n, np.int32), np.zeros(n, np.float32)
        _check(self.L.crh_render_adaptive(self.h, C.byref(p), arr, n, C.byref(a), fb, half, count.ctypes.data, errors.ctypes.data), "crh_render_adaptive")
        return count, errors

    # ---- ... at cell granularity within each rectangle (crh_adaptive_step_cells, crh_render_adaptive_cells) ----
    def adaptive_step_cells(self, fb, half, width, height, tiles, cell, threshold, dilate=0, live=None):
        """One step over the cells of `tiles` (adaptive_cell_offsets gives their order): (errors float32 [cells], flags bool [cells]). A live cell goes on when its
        error is not <= threshold or, with dilate, when that holds for one of its neighbours in the same rectangle; where it goes on, half := fb over it.
        live: one truth value per cell (None: all). Waits for the result. threshold = inf measures only."""
        n = len(tiles)
        total = int(adaptive_cell_offsets(tiles, cell)[-1])
        arr = _tile_array(tiles)
        errors, flags = np.zeros(total, np.float32), np.zeros(total, np.uint8)
        mask = None
        if live is not None:
            mask = np.ascontiguousarray(np.asarray(live).astype(bool).astype(np.uint8))
            if mask.shape != (total,):
                raise ValueError(f"adaptive_step_cells(): live has shape {mask.shape}, the rectangles hold {total} cells")
        _check(self.L.crh_adaptive_step_cells(self.h, fb, half, width, height, arr, n, cell, threshold, int(dilate), None if mask is None else mask.ctypes.data,
                                              errors.ctypes.data, flags.ctypes.data), "crh_adaptive_step_cells")
        return errors, flags.astype(bool)

    def render_adaptive_cells(self, fb, half, width, height, max_samples, bounces, tiles, min_passes=16, threshold=0.05, cell=16, dilate=1, passes=None):
        """crh_render_adaptive_cells: render_adaptive with the cell as the unit of decision inside every rectangle. Returns (passes per cell int32 [cells], error per
        cell float32 [cells]) in adaptive_cell_offsets' order; fb holds each cell's mean of its passes, half the mean of the first half of them."""
        n = len(tiles)
        total = int(adaptive_cell_offsets(tiles, cell)[-1])
        p = abi.RenderParams(0, 0, 0, 0, width, height, 0, max_samples if passes is None else passes, max_samples, bounces)
        a = abi.AdaptiveCellsParams(min_passes, threshold, cell, int(dilate))
        arr = _tile_array(tiles)
        count, errors = np.zeros(total, np.int32), np.zeros(total, np.float32)
        _check(self.L.crh_render_adaptive_cells(self.h, C.byref(p), arr, n, C.byref(a), fb, half, count.ctypes.data, errors.ctypes.data), "crh_render_adaptive_cells")
        return count, errors

    def adaptive_time_ms(self):
        """Milliseconds of the most recent adaptive step's kernel (render_adaptive's count); 0.0 before the first one."""
        ms = C.c_float(0.0)
        _check(self.L.crh_adaptive_time_ms(self.h, C.byref(ms)), "crh_adaptive_time_ms")
        return float(ms.value)

    def denoise_time_ms(self):
        """Milliseconds of the most recent denoise() or denoise_variance(), summed over its launches (waits for it); 0.0 before the first one."""
        ms = C.c_float(0.0)
        _check(self.L.crh_denoise_time_ms(self.h, C.byref(ms)), "crh_denoise_time_ms")
        return float(ms.value)

    def denoise_launch_ms(self):
        """... launch by launch: [prepare, iteration 0, iteration 1, ...]; after denoise_variance() [prepare, prefilter, iteration 0, ...] (crh_debug_denoise_launch_ms)."""
        ms = (C.c_float * 16)()
        n = self.L.crh_debug_denoise_launch_ms(self.h, ms, 16)
        if n < 0:
            _check(n, "crh_debug_denoise_launch_ms")
        return [float(ms[i]) for i in range(n)]

    def synchronize(self):
        _check(self.L.crh_synchronize(self.h), "crh_synchronize")

    def download(self, fb, width, height):
        out = np.empty((height, width, 3), dtype=np.float32)
        _check(self.L.crh_framebuffer_download(self.h, fb, width, height, out.ctypes.data), "crh_framebuffer_download")
        return out

    def to_srgb8(self, fb, width, height):
        out = np.empty((height, width, 3), dtype=np.uint8)
        _check(self.L.crh_framebuffer_to_srgb8(self.h, fb, width, height, out.ctypes.data), "crh_framebuffer_to_srgb8")
        return out

    def counters(self):
        c = abi.Counters()
        _check(self.L.crh_counters_get(self.h, C.byref(c)), "crh_counters_get")
        return c.as_dict()

    def reset_counters(self):
        _check(self.L.crh_counters_reset(self.h), "crh_counters_reset")

    def kernel_time_ms(self):
        last, total, n = C.c_float(), C.c_double(), C.c_uint64()
        _check(self.L.crh_kernel_time_ms(self.h, C.byref(last), C.byref(total), C.byref(n)), "crh_kernel_time_ms")
        return last.value, total.value, n.value

    def strips_to_srgb8(self, fb, width, height, strip_rows, g, n_gpus, out):
        """crh_framebuffer_strips_to_srgb8: the rows of GPU g's strips of the 8-bit frame into `out` (uint8 [height, width, 3]); the other rows stay as they are."""
        _check(self.L.crh_framebuffer_strips_to_srgb8(self.h, fb, width, height, strip_rows, g, n_gpus, out.ctypes.data), "crh_framebuffer_strips_to_srgb8")
        return out

    def last_kernel_name(self):
        """The instantiation of the path-tracing kernel launched last, as a profiler names it ("" before the first dispatch)."""
        return (self.L.crh_last_kernel_name(self.h) or b"").decode()

    def bvh_build_triangles(self, polys_ptr, poly_count, vertices_ptr, vertex_count):
        """buildBottomLevelBvh on the GPU: (nodes uint32[n, 8] = crh_bvh_node records, prim order int32[count], stats dict)."""
        nodes = np.zeros((max(2 * poly_count - 1, 1), 8), np.uint32)
        prims = np.zeros(max(poly_count, 1), np.int32)
        n = C.c_uint32(0)
        st = abi.BvhBuildStats()
        _check(self.L.crh_bvh_build_triangles(self.h, polys_ptr, poly_count, vertices_ptr, vertex_count, nodes.ctypes.data,
                                              prims.ctypes.data, C.byref(n), C.byref(st)), "crh_bvh_build_triangles")
        return nodes[:n.value], prims[:poly_count], {k: getattr(st, k) for k, _ in abi.BvhBuildStats._fields_ if k != "pad"}

    def frames_reduce(self, fb, width, height):
        """crh_frames_reduce over this one context (n = 1: a no-op unless CRH_FORCE_RCCL is set)."""
        ctxs = (C.c_void_p * 1)(self.h)
        fbs = (C.c_void_p * 1)(fb)
        _check(self.L.crh_frames_reduce(ctxs, fbs, 1, width, height), "crh_frames_reduce")

    def eval_math(self, function, x, y=None):
        """crh_debug_eval_math: the device build of exact_math.h on caller values (function = a name from abi.MATH_FUNCTIONS)."""
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        out = np.empty_like(x)
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float32).ravel()
            assert y.size == x.size
            yp = y.ctypes.data
        _check(self.L.crh_debug_eval_math(self.h, abi.MATH_FUNCTIONS.index(function), x.ctypes.data, yp, x.size, out.ctypes.data), "crh_debug_eval_math")
        return out

    # ---- round 6: the walk-only probe (debug / measurement; include/cray_hip.h) ----
    def ray_dump(self, rays_per_wave):
        _check(self.L.crh_debug_ray_dump(self.h, rays_per_wave), "crh_debug_ray_dump")

    def ray_dump_counts(self, max_waves=8192):
        total = C.c_uint64(0)
        per = np.zeros(max_waves, dtype=np.uint32)
        _check(self.L.crh_debug_ray_dump_counts(self.h, C.byref(total), per.ctypes.data, max_waves), "crh_debug_ray_dump_counts")
        return int(total.value), per

    def ray_dump_fetch(self, wave, first, n):
        out = np.zeros((n, 6), dtype=np.float32)
        _check(self.L.crh_debug_ray_dump_fetch(self.h, wave, first, n, out.ctypes.data), "crh_debug_ray_dump_fetch")
        return out

    def walk_probe(self, wps, stack_lds=12, inst_lds=True, fused=True, unit_rays=512, slot=0):
        """-> (kernel ms, rays walked)"""
        ms = C.c_float(0.0)
        rays = C.c_uint64(0)
        _check(self.L.crh_debug_walk_probe(self.h, wps, stack_lds, 1 if inst_lds else 0, int(fused), unit_rays, slot, C.byref(ms), C.byref(rays)), "crh_debug_walk_probe")
        return float(ms.value), int(rays.value)

    def walk_probe_fetch(self, slot, wave, first, n):
        hits = np.zeros((n, 4), dtype=np.float32)
        inst = np.zeros(n, dtype=np.int32)
        _check(self.L.crh_debug_walk_probe_fetch(self.h, slot, wave, first, n, hits.ctypes.data, inst.ctypes.data), "crh_debug_walk_probe_fetch")
        return hits, inst

    def walk_probe_compare(self):
        d = C.c_uint64(0)
        _check(self.L.crh_debug_walk_probe_compare(self.h, C.byref(d)), "crh_debug_walk_probe_compare")
        return int(d.value)

    def trace_rays(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        hits = np.zeros(len(rays), dtype=abi.HIT_DTYPE)
        _check(self.L.crh_trace_rays(self.h, rays.ctypes.data, len(rays), hits.ctypes.data), "crh_trace_rays")
        return hits
