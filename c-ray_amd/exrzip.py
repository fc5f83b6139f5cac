"""exrzip.py — thin ctypes binding of libcray_hip_exr.so (include/cray_hip_exr.h), the companion library of output codecs: the pixel data of a ZIP / ZIPS
compressed scanline OpenEXR file, deflated on the device, FLOAT or per channel HALF, and the 8-bit frame as a complete PNG file (ZipContext.png), optionally through a display
transform (display=: exposure, tone curve, dither) at an exposure the device measures (ZipContext.auto_exposure); and, no codec but at home here because it needs
no scene, the firefly filter in front of the denoisers (ZipContext.despeckle). Plumbing: the work
is in c-ray_amd/csrc/exr_zip.h, png_pack.h, png_display.h and despeckle.h. The library loads on first use; there is no CPU
fallback: `library()` raises if it has not been built, every call raises `CrhError` on a non-zero return code.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .api import CrhError

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CRX_LIB") or os.path.join(HERE, "_lib", "libcray_hip_exr.so")    # CRX_LIB: another build (dev, the emulation tier)
COMPRESSION = {"none": (0, 1), "zips": (2, 1), "zip": (3, 16)}          # name -> (the file's compression attribute, lines per chunk)
CODES = {"fixed": 0, "dynamic": 1}          # name -> CRX_CODES_*
PNG_FILTERS = {"adaptive": -1, "none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4}          # name -> crx_png_pack's filter
PNG_PHASES = ("convert", "filter", "deflate", "crc + scan", "emit")
CURVES = {"clamp": 0, "reinhard": 1, "aces": 2, "hable": 3}          # name -> CRX_CURVE_*


class PngText(C.Structure):
    """crx_png_text: a tEXt chunk"""
    _fields_ = [("key", C.c_char_p), ("value", C.c_char_p)]


class Display(C.Structure):
    """crx_display: the display transform of crx_png_pack_display"""
    _fields_ = [("exposure", C.c_float), ("curve", C.c_int), ("white", C.c_float), ("dither", C.c_int)]


class DespeckleParams(C.Structure):
    """crx_despeckle_params: the firefly filter's rule"""
    _fields_ = [("radius", C.c_int), ("rank", C.c_int), ("factor", C.c_float), ("floor", C.c_float)]


class DespeckleStats(C.Structure):
    """crx_despeckle_stats"""
    _fields_ = [("clamped", C.c_uint64), ("bad", C.c_uint64), ("max_clamped", C.c_float), ("min_scale", C.c_float)]


def display_of(display):
    """The crx_display of `display`: a Display, None (the default: 1, clamp, 4, no dither) or a mapping with any of exposure, curve (a name of CURVES or its number),
    white, dither. An unknown curve name or key raises ValueError; whether the values are in range is the library's to say."""
    if isinstance(display, Display):
        return display
    d = Display()
    library().crx_display_default(C.byref(d))
    for key, value in dict(display or {}).items():
        if key not in ("exposure", "curve", "white", "dither"):
            raise ValueError(f"display: unknown key {key!r}")
        if key == "curve" and isinstance(value, str):
            if value not in CURVES:
                raise ValueError(f"curve {value!r}: one of {sorted(CURVES)}")
            value = CURVES[value]
        setattr(d, key, int(value) if key in ("curve", "dither") else float(value))
    return d


def png_texts(text):
    """(the crx_png_text array or None, its count) of `text`: a mapping or an iterable of (key, value), str (stored as Latin-1) or bytes."""
    pairs = list(text.items()) if hasattr(text, "items") else list(text or ())
    raw = [tuple(s if isinstance(s, bytes) else str(s).encode("latin-1") for s in kv) for kv in pairs]
    if any(len(kv) != 2 or b"\0" in kv[0] or b"\0" in kv[1] for kv in raw):
        raise ValueError("text: (key, value) pairs without NUL bytes")
    arr = (PngText * len(raw))(*[PngText(k, v) for k, v in raw]) if raw else None
    return arr, len(raw)

_lib = None


def library():
    """Load libcray_hip_exr.so (built by c-ray_amd/build.py). Raises loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} is missing: run `python c-ray_amd/build.py` (or __graft_entry__.build()); there is no CPU fallback")
    try:          # (as api.library(): torch's copy of the HIP runtime first, where there is one)
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    if hasattr(L, "crx_emu_stats") and os.environ.get("CRH_ALLOW_EMULATION") != "1":
        raise RuntimeError(f"{LIB_PATH} is the CPU emulation of the kernels (test infrastructure): the product has no CPU path "
                           "(set CRH_ALLOW_EMULATION=1 only in tests / tools that mean it)")
    ctx = C.c_void_p
    sig = {
        "crx_context_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(ctx)]),
        "crx_context_destroy": (C.c_int, [ctx]),
        "crx_last_error": (C.c_char_p, []),
        "crx_pack_zip": (C.c_int, [ctx, C.POINTER(abi.PackChannel), C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
        "crx_pack": (C.c_int, [ctx, C.POINTER(abi.PackChannel), C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
        "crx_pack_zip_time_ms": (C.c_int, [ctx, C.POINTER(C.c_float)]),
        "crx_pack_zip_phases_ms": (C.c_int, [ctx, C.POINTER(C.c_float)]),
        "crx_zip_segment_bytes": (C.c_uint32, []),
        "crx_set_codes": (C.c_int, [ctx, C.c_int]),
        "crx_get_codes": (C.c_int, [ctx, C.POINTER(C.c_int)]),
        "crx_debug_code_lengths": (C.c_int, [ctx, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
        "crx_png_bound": (C.c_int, [C.c_int, C.c_int, C.POINTER(PngText), C.c_uint32, C.POINTER(C.c_uint64)]),
        "crx_png_pack": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(PngText), C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "crx_png_phases_ms": (C.c_int, [ctx, C.POINTER(C.c_float)]),
        "crx_display_default": (None, [C.POINTER(Display)]),
        "crx_png_pack_display": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int, C.POINTER(Display), C.c_int, C.POINTER(PngText), C.c_uint32, C.c_void_p, C.c_uint64,
                                           C.POINTER(C.c_uint64)]),
        "crx_auto_exposure": (C.c_int, [ctx, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64)]),
        "crx_auto_exposure_time_ms": (C.c_int, [ctx, C.POINTER(C.c_float)]),
        "crx_debug_crc32": (C.c_int, [ctx, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)]),
        "crx_despeckle_default": (None, [C.POINTER(DespeckleParams)]),
        "crx_despeckle": (C.c_int, [ctx, C.POINTER(DespeckleParams), C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(DespeckleStats)]),
        "crx_despeckle_scale": (C.c_int, [ctx, C.c_void_p]),
        "crx_despeckle_time_ms": (C.c_int, [ctx, C.POINTER(C.c_float)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _check(rc, where):
    if rc != 0:
        raise CrhError(rc, where, (library().crx_last_error() or b"").decode(errors="replace"))


def segment_bytes():
    return int(library().crx_zip_segment_bytes())


class ZipContext:
    """One crx_ctx: a device, a stream (a raw hipStream_t, or None for one of the library's own) and the scratch of its calls."""

    def __init__(self, device=0, stream=None):
        self.L = library()
        self.h = C.c_void_p()
        _check(self.L.crx_context_create(int(device), C.c_void_p(stream) if stream else None, C.byref(self.h)), "crx_context_create")

    def close(self):
        if self.h:
            self.L.crx_context_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_codes(self, codes):
        """Which Huffman codes the deflate blocks of the following calls use (crx_set_codes): "fixed" — the default, the bytes there have always been — or
        "dynamic": per segment the cheaper of the fixed codes and a dynamic code built on the device from the segment's own counts. Sticky on the context."""
        if codes not in CODES:
            raise ValueError(f"codes {codes!r}: one of {sorted(CODES)}")
        _check(self.L.crx_set_codes(self.h, CODES[codes]), "crx_set_codes")

    @property
    def codes(self):
        value = C.c_int(-1)
        _check(self.L.crx_get_codes(self.h, C.byref(value)), "crx_get_codes")
        return {v: k for k, v in CODES.items()}[value.value]

    def code_lengths(self, freq, limit):
        """crx_debug_code_lengths: the deflate kernel's code construction on histograms of the caller's — `freq` [count, symbols] or [symbols] counts, `limit` 7 or
        15 bits — gives the uint8 array of code lengths, shaped like freq."""
        f = np.ascontiguousarray(freq, dtype=np.uint32)
        if f.ndim not in (1, 2) or f.size == 0:
            raise ValueError("freq: [symbols] or [count, symbols] counts")
        out = np.zeros(f.shape, np.uint8)
        _check(self.L.crx_debug_code_lengths(self.h, f.ctypes.data, f.shape[-1], int(limit), f.size // f.shape[-1], out.ctypes.data), "crx_debug_code_lengths")
        return out

    def _pack(self, where, call, channels, pixel_bytes, width, lines_per_chunk, rows):
        """One call of the pack entry named `where` — call(the crh_pack_channel array, output, sizes, total) -> its return code — with the output sized to its bound,
        8 bytes a chunk + the raw bytes (pixel_bytes: the sum of the channels' pixel sizes): (the chunks as bytes, the uint64 array of their byte counts)."""
        arr, keep = abi.pack_channels(channels)
        chunks = max(-(-max(rows, 0) // max(lines_per_chunk, 1)), 0)
        out = np.empty(8 * chunks + pixel_bytes * max(width, 0) * max(rows, 0), np.uint8)
        sizes = np.zeros(max(chunks, 1), np.uint64)
        total = C.c_uint64(0)
        _check(call(arr, out.ctypes.data, sizes.ctypes.data, C.byref(total)), where)
        del keep
        return out[:total.value].tobytes(), sizes[:chunks if total.value else 0]

    def pack_zip(self, channels, width, height, lines_per_chunk, first_row=0, row_count=None):
        """(the chunks of stored rows [first_row, first_row + row_count) as bytes — per chunk int32 y, int32 size, the data —, the uint64 array of their byte
        counts). Channels as Context.pack_scanlines takes them; lines_per_chunk 1 (ZIPS) or 16 (ZIP). The sources must be complete."""
        n, rows = len(channels), height - first_row if row_count is None else row_count
        return self._pack("crx_pack_zip", lambda arr, *out: self.L.crx_pack_zip(self.h, arr, n, width, height, first_row, rows, lines_per_chunk, *out),
                          channels, 4 * n, width, lines_per_chunk, rows)

    def pack(self, channels, width, height, compression, pixel_types=None, first_row=0, row_count=None):
        """pack_zip with a pixel type per channel (crx_pack): `compression` is the file's attribute — 0 none (a raw chunk a row), 2 ZIPS, 3 ZIP — or its name in
        COMPRESSION, `pixel_types` 0 (FLOAT: the word as it is) or 1 (HALF: the word's binary16 conversion, round to nearest even; values above 65504 become infinity) per channel, None
        for all FLOAT. Returns (the chunks as bytes, the uint64 array of their byte counts)."""
        compression = COMPRESSION[compression][0] if isinstance(compression, str) else int(compression)
        n, rows = len(channels), height - first_row if row_count is None else row_count
        types = None if pixel_types is None else np.ascontiguousarray(pixel_types, dtype=np.uint8)
        if types is not None and types.shape != (n,):
            raise ValueError("pixel_types: one entry per channel")
        return self._pack("crx_pack", lambda arr, *out: self.L.crx_pack(self.h, arr, None if types is None else types.ctypes.data, n, width, height, first_row, rows, compression, *out),
                          channels, 4 * n if types is None else int(np.where(types == 1, 2, 4).sum()), width, 16 if compression == 3 else 1, rows)

    def png(self, fb, width, height, filter="adaptive", text=(), display=None):
        """crx_png_pack: the bytes of a complete PNG file of the device frame `fb` ([height, width, 3] floats, complete) — 8-bit sRGB, the bytes of
        Context.to_srgb8, filtered and deflated on the device under the context's codes setting. filter: a name of PNG_FILTERS ("adaptive": per row the type with
        the least sum of min(v, 256 - v)) or its number -1 .. 4; text: tEXt chunks, a mapping or (key, value) pairs, Latin-1, keys of 1 .. 79 bytes. display: None —
        crx_png_pack, as ever — or what display_of takes: exposure, a tone curve of CURVES, its white point and the ordered dither between the float and the
        byte (crx_png_pack_display; the default display gives crx_png_pack's bytes)."""
        if isinstance(filter, str):
            if filter not in PNG_FILTERS:
                raise ValueError(f"filter {filter!r}: one of {sorted(PNG_FILTERS)}")
            filter = PNG_FILTERS[filter]
        arr, count = png_texts(text)
        bound, total = C.c_uint64(0), C.c_uint64(0)
        _check(self.L.crx_png_bound(width, height, arr, count, C.byref(bound)), "crx_png_bound")
        out = np.empty(bound.value, np.uint8)
        if display is None:
            _check(self.L.crx_png_pack(self.h, fb, width, height, int(filter), arr, count, out.ctypes.data, bound.value, C.byref(total)), "crx_png_pack")
        else:
            d = display_of(display)
            _check(self.L.crx_png_pack_display(self.h, fb, width, height, C.byref(d), int(filter), arr, count, out.ctypes.data, bound.value, C.byref(total)),
                   "crx_png_pack_display")
        return out[:total.value].tobytes()

    def auto_exposure(self, fb, width, height, permille=500, target=0.18):
        """crx_auto_exposure: (exposure, key, counted) of the device frame `fb` — the exposure, as np.float32, that takes the bin midpoint `key` of the
        permille / 1000 quantile of the pixels' luminances to `target`, limited to [2^-40, 2^40]; `counted` pixels have a finite luminance > 0. No such pixel:
        (1, 0, 0). A function of the pixels and the arguments only."""
        exposure, key, counted = C.c_float(0.0), C.c_float(0.0), C.c_uint64(0)
        _check(self.L.crx_auto_exposure(self.h, fb, width, height, int(permille), float(target), C.byref(exposure), C.byref(key), C.byref(counted)), "crx_auto_exposure")
        return np.float32(exposure.value), np.float32(key.value), int(counted.value)

    def auto_exposure_time_ms(self):
        """Milliseconds of the most recent auto_exposure's two kernels (waits for them)."""
        ms = C.c_float(0.0)
        _check(self.L.crx_auto_exposure_time_ms(self.h, C.byref(ms)), "crx_auto_exposure_time_ms")
        return float(ms.value)

    def despeckle(self, guide, width, height, frames=(), **params):
        """crx_despeckle: the firefly filter. Measures from the device frame `guide` ([height, width, 3] floats, complete) the plane of scales that takes every
        pixel brighter than factor * (the rank-th largest luminance of its neighbours within radius) + floor down to that limit, and multiplies every device frame
        of `frames` (at most 8; `guide` may be among them) by it IN PLACE; without frames it only measures. params: radius, rank, factor, floor
        (crx_despeckle_default otherwise: 2, 4, 4, 2^-6); an unknown name raises TypeError. Returns the stats: clamped and bad pixel counts, max_clamped (the
        largest luminance clamped, 0 if none) and min_scale (the smallest scale of a clamped pixel, 1 if none), the floats as np.float32. Waits."""
        p = DespeckleParams()
        self.L.crx_despeckle_default(C.byref(p))
        for k, v in params.items():
            if k not in ("radius", "rank", "factor", "floor"):
                raise TypeError(f"despeckle() got an unexpected parameter {k!r}")
            setattr(p, k, int(v) if k in ("radius", "rank") else float(v))
        frames = list(frames)
        arr = (C.c_void_p * max(len(frames), 1))(*frames)
        stats = DespeckleStats()
        _check(self.L.crx_despeckle(self.h, C.byref(p), guide, width, height, arr if frames else None, len(frames), C.byref(stats)), "crx_despeckle")
        self._despeckled = (int(width), int(height))
        return dict(clamped=int(stats.clamped), bad=int(stats.bad), max_clamped=np.float32(stats.max_clamped), min_scale=np.float32(stats.min_scale))

    def despeckle_scale(self, width, height):
        """crx_despeckle_scale: the plane of scales of the last despeckle() on this context, float32 [height, width] — its own size, anything else raises
        ValueError: 1 where the pixel stayed, 0 where it was bad, the factor below 1 where it was clamped."""
        if getattr(self, "_despeckled", None) != (int(width), int(height)):
            raise ValueError(f"despeckle_scale({width}, {height}): the last despeckle() on this context was {getattr(self, '_despeckled', None)}")
        out = np.empty((height, width), np.float32)
        _check(self.L.crx_despeckle_scale(self.h, out.ctypes.data), "crx_despeckle_scale")
        return out

    def despeckle_time_ms(self):
        """Milliseconds of the most recent despeckle(): (the measure kernel, the apply kernels summed over the frames); waits for them."""
        ms = (C.c_float * 2)()
        _check(self.L.crx_despeckle_time_ms(self.h, ms), "crx_despeckle_time_ms")
        return float(ms[0]), float(ms[1])

    def png_phases_ms(self):
        """Milliseconds per phase of the most recent png(): convert, filter, deflate, crc + scan, emit (PNG_PHASES; waits for it)."""
        ms = (C.c_float * len(PNG_PHASES))()
        _check(self.L.crx_png_phases_ms(self.h, ms), "crx_png_phases_ms")
        return [float(v) for v in ms]

    def crc32(self, data, piece_bytes):
        """crx_debug_crc32: the CRC-32 of `data` taken on the device in pieces of piece_bytes and combined there — zlib.crc32(data), whatever the pieces."""
        data = bytes(data)
        crc = C.c_uint32(0)
        _check(self.L.crx_debug_crc32(self.h, data if data else None, len(data), int(piece_bytes), C.byref(crc)), "crx_debug_crc32")
        return int(crc.value)

    def time_ms(self):
        """Milliseconds of the most recent pack_zip's kernels, summed (waits for them)."""
        ms = C.c_float(0.0)
        _check(self.L.crx_pack_zip_time_ms(self.h, C.byref(ms)), "crx_pack_zip_time_ms")
        return float(ms.value)

    def phases_ms(self):
        """Milliseconds per launch of the most recent pack_zip: gather + transform, deflate, sizes and offsets, compaction."""
        ms = (C.c_float * 4)()
        _check(self.L.crx_pack_zip_phases_ms(self.h, ms), "crx_pack_zip_phases_ms")
        return [float(v) for v in ms]
