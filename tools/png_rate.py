#!/usr/bin/env python3
"""png_rate.py — what the PNG of the 8-bit frame costs when it is filtered, deflated and check-summed on the device (crx_png_pack), beside host encoders on the
same pixels.

    python tools/png_rate.py [--blob scenes/_built/cfg2_hdr.blob] [--size 1280x720] [--passes 16] [--bounces 8] [--display] [--out profiles/png_rate.log]

The blob's scene is rendered at the size (the blob's own aspect ratio is the caller's business), `passes` passes. Then, in one process, behind warm-up rounds, medians
of interleaved rounds of ZipContext.png for filter "adaptive" under dynamic and under fixed codes: the five phases by crx_png_phases_ms (the companion library's
events around its launches), and the wall time of the whole call (header upload, kernels, size, copy through pinned memory, copy out). Once each: the file size under
both code settings for "adaptive" and each fixed filter type. The host yardsticks, once each on one thread, on the same pixels: to_srgb8's download + PIL's PNG encoder
at compress_level 1 and 6 (time and size), and zlib level 1 and 6 over the device's own filtered bytes F (time and size of the stream) — the second says what the
4 096-byte segments and the parse cost against zlib's 32 KB window on identical input. With --display, between the two: the display transform (measure_display: every
curve with and without the dither against png() of the same interleaved rounds, and crx_auto_exposure). Nothing is asserted; without a GPU nothing is measured and the log says so."""
import io
import os
import statistics
import struct
import sys
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, WARM = 7, 2


def idat_of(data):
    """the IDAT payload of a PNG file with one IDAT"""
    at = 8
    while at < len(data):
        (size,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        if kind == b"IDAT":
            return data[at + 8:at + 8 + size]
        at += 12 + size
    raise ValueError("no IDAT")


def measure_display(zctx, exrzip, fb, w, h):
    """--display: the display transform's cost. Interleaved rounds, under dynamic codes, of png() — the parent's call, the yardstick — and png(display=...) for each
    curve with and without the dither at the exposure crx_auto_exposure measures, and of auto_exposure itself: the convert phase and the whole call's wall time
    per variant, the two kernels' time and the call's wall time for the exposure."""
    exposure, key, counted = zctx.auto_exposure(fb, w, h)
    lines = [f"display transform (--display): auto exposure {float(exposure):.9g} (key {float(key):.9g}, {counted} of {w * h} pixels count); dynamic codes, filter adaptive"]
    variants = [("png() without a display", None)] + [(f"{curve:8s} dither {dither}", dict(exposure=float(exposure), curve=curve, dither=dither))
                                                      for curve in exrzip.CURVES for dither in (0, 1)]
    t = {name: {"call": [], "convert": [], "sum": []} for name, _ in variants}
    auto = {"call": [], "kernels": []}
    zctx.set_codes("dynamic")
    for r in range(WARM + ROUNDS):
        for name, display in variants:
            t0 = time.perf_counter()
            zctx.png(fb, w, h, "adaptive", display=display)
            t1 = time.perf_counter()
            if r >= WARM:
                phases = zctx.png_phases_ms()
                t[name]["call"].append((t1 - t0) * 1e3); t[name]["convert"].append(phases[0]); t[name]["sum"].append(sum(phases))
        t0 = time.perf_counter()
        zctx.auto_exposure(fb, w, h)
        t1 = time.perf_counter()
        if r >= WARM:
            auto["call"].append((t1 - t0) * 1e3); auto["kernels"].append(zctx.auto_exposure_time_ms())
    zctx.set_codes("fixed")
    base = statistics.median(t[variants[0][0]]["call"])
    for name, _ in variants:
        call, conv = t[name]["call"], t[name]["convert"]
        lines.append(f"  {name:24s}: convert {statistics.median(conv):.4f} ms (min {min(conv):.4f}, max {max(conv):.4f}); kernels {statistics.median(t[name]['sum']):.3f} ms; "
                     f"whole call (wall) median {statistics.median(call):.3f} ms (min {min(call):.3f}, max {max(call):.3f}) = {statistics.median(call) - base:+.3f} ms against png()")
    lines.append(f"  crx_auto_exposure       : kernels (histogram + pick) median {statistics.median(auto['kernels']):.4f} ms (min {min(auto['kernels']):.4f}, max {max(auto['kernels']):.4f}); "
                 f"whole call (wall) median {statistics.median(auto['call']):.3f} ms (min {min(auto['call']):.3f}, max {max(auto['call']):.3f})")
    return lines


def measure(blob, w, h, passes, bounces, display=False):
    sys.path.insert(0, REPO)
    from PIL import Image
    from __graft_entry__ import load_package
    pkg = load_package()
    api = pkg.api
    import cray_amd.exrzip as exrzip
    ctx = api.Context(0)
    ctx.upload(api.Scene(blob))
    fb = ctx.framebuffer(w, h)
    ctx.render_region(fb, w, h, passes, bounces)
    ctx.synchronize()
    zctx = exrzip.ZipContext(0)
    n = (3 * w + 1) * h
    lines = [f"{os.path.basename(blob)} {w}x{h}, {passes} passes: {3 * w * h} bytes of pixels, n = {n} filtered bytes in {-(-n // exrzip.segment_bytes())} segments of "
             f"{exrzip.segment_bytes()}; {ROUNDS} interleaved rounds behind {WARM} warm-up rounds, one process, one device"]
    t = {c: {"call": [], "phases": []} for c in exrzip.CODES}
    for r in range(WARM + ROUNDS):
        for codes in t:
            zctx.set_codes(codes)
            t0 = time.perf_counter()
            zctx.png(fb, w, h, "adaptive")
            t1 = time.perf_counter()
            if r >= WARM:
                t[codes]["call"].append((t1 - t0) * 1e3)
                t[codes]["phases"].append(zctx.png_phases_ms())
    for codes in t:
        ph = np.median(np.array(t[codes]["phases"]), axis=0)
        call = t[codes]["call"]
        lines.append(f"adaptive, {codes:7s} codes: kernels (crx_png_phases_ms): " + ", ".join(f"{name} {v:.3f} ms" for name, v in zip(exrzip.PNG_PHASES, ph)) +
                     f"; sum {ph.sum():.3f} ms; whole call (wall) median {statistics.median(call):.3f} ms (min {min(call):.3f}, max {max(call):.3f})")
    if display:
        lines += measure_display(zctx, exrzip, fb, w, h)
    size, idat, filtered = {}, {}, None
    for name in exrzip.PNG_FILTERS:
        for codes in exrzip.CODES:
            zctx.set_codes(codes)
            data = zctx.png(fb, w, h, name)
            size[name, codes] = len(data)
            if name == "adaptive":
                idat[codes] = len(idat_of(data))
                filtered = zlib.decompress(idat_of(data))
        lines.append(f"filter {name:8s}: file {size[name, 'fixed']:9d} bytes under fixed codes, {size[name, 'dynamic']:9d} under dynamic = {size[name, 'dynamic'] / (3 * w * h):.4f} of the pixels")
    zctx.set_codes("fixed")
    own = size["adaptive", "dynamic"]
    t0 = time.perf_counter()
    rgb8 = ctx.to_srgb8(fb, w, h)
    down = (time.perf_counter() - t0) * 1e3
    lines.append(f"host yardsticks, one thread, on the same pixels (Context.to_srgb8: conversion on the device + download {down:.1f} ms, in none of the times below):")
    image = Image.fromarray(rgb8, "RGB")
    for level in (1, 6):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        image.save(buf, "PNG", compress_level=level)
        pil_ms = ms = (time.perf_counter() - t0) * 1e3
        lines.append(f"  PIL PNG encoder, compress_level {level}: {ms:8.1f} ms, {buf.tell():9d} bytes; the device's file (adaptive, dynamic) is {own / buf.tell():.4f} of it")
    for level in (1, 6):
        t0 = time.perf_counter()
        z = zlib.compress(filtered, level)
        ms = (time.perf_counter() - t0) * 1e3
        lines.append(f"  zlib level {level} over the device's F (adaptive): {ms:8.1f} ms, {len(z):9d} bytes; the device's IDAT data: dynamic {idat['dynamic']} = {idat['dynamic'] / len(z):.4f} of it, "
                     f"fixed {idat['fixed']} = {idat['fixed'] / len(z):.4f} of it")
    call6 = statistics.median(t["dynamic"]["call"])
    lines.append(f"time against PIL at compress_level 6 on this host's CPU: the device's whole call (adaptive, dynamic codes) takes {call6:.3f} ms against {pil_ms:.1f} ms = {pil_ms / call6:.0f} x")
    zctx.close()
    ctx.close()
    return lines


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return args[args.index(name) + 1] if name in args else default
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from __graft_entry__ import load_package
    from denoise_rate import blob_path
    w, h = (int(v) for v in opt("--size", "1280x720").split("x"))
    out = opt("--out", os.path.join(REPO, "profiles", "png_rate.log"))
    gpu = load_package().api.device_count() > 0
    lines = (measure(opt("--blob", None) or blob_path(), w, h, int(opt("--passes", "16")), int(opt("--bounces", "8")), "--display" in args) if gpu
             else ["no HIP device here: nothing is measured"])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
