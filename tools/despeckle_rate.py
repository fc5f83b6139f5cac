#!/usr/bin/env python3
"""despeckle_rate.py — what the firefly filter (crx_despeckle) costs, and what it does to pictures in front of the two denoisers.

    python tools/despeckle_rate.py [--sizes 1280x720,3840x2160] [--picture-size 1280x720] [--out profiles/despeckle_rate.log]

Time. scenes/_built/cfg2_hdr.blob is rendered at each size, 4 passes (a frame with real fireflies). In one process, behind warm-up rounds, medians of interleaved
rounds: the measure kernel and the apply kernel on one and on two frames by crx_despeckle_time_ms (the companion library's events around its launches), the whole
call's wall time, and — the yardstick — crh_framebuffer_copy of the same frame (20 copies back to back and one wait, wall time / 20: the copy reads what measure
reads and streams what a plain apply would stream). Every round works on a fresh copy of the frame: the filter changes its input.

Pictures. cfg2_hdr and cfg3_venus at the picture size, 16 and 64 passes, against the same scene at 256 passes: the clamped share, the share of the luminance the
filter removes, and the RMSE against the 256-pass frame of the frame, of the denoised frame and of the despeckled-then-denoised frame, for crh_denoise and for
crh_denoise_variance (the half-sample buffer scaled by the same plane). Two RMSEs each: of the linear values, and of x / (1 + x), which a handful of pixels in the
hundreds do not decide. Last, the defaults on the 4-pass frames of cfg2_hdr, cfg3_venus and cfg4_statues.
Nothing is asserted; without a GPU nothing is measured and the log says so."""
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, WARM, COPIES = 9, 3, 20
SCENES = {"cfg2_hdr": 8, "cfg3_venus": 32, "cfg4_statues": 30}          # blob -> bounces (__graft_entry__.BLOBS)


def blob(name):
    p = os.path.join(REPO, "scenes", "_built", name + ".blob")
    return p if os.path.exists(p) else None


def lum(a):
    L = (np.float32(0.2126) * a[..., 0] + np.float32(0.7152) * a[..., 1]) + np.float32(0.0722) * a[..., 2]
    return np.where(np.isfinite(L) & (L > 0), L, 0).astype(np.float64)


def rmse2(a, ref):
    """(linear RMSE, RMSE of x / (1 + x)) over finite, non-negative values"""
    a, ref = np.nan_to_num(np.maximum(a, 0), posinf=0).astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(np.mean((a - ref) ** 2))), float(np.sqrt(np.mean((a / (1 + a) - ref / (1 + ref)) ** 2)))


def measure_time(api, exrzip, w, h):
    ctx = api.Context(0)
    ctx.upload(api.Scene(blob("cfg2_hdr")))
    fb, work, other = ctx.framebuffer(w, h), ctx.framebuffer(w, h), ctx.framebuffer(w, h)
    ctx.render_region(fb, w, h, 4, SCENES["cfg2_hdr"])
    ctx.synchronize()
    z = exrzip.ZipContext(0)
    t = {k: [] for k in ("measure", "apply1", "apply2", "call1", "copy")}
    stats = None
    for r in range(WARM + ROUNDS):
        ctx.copy_framebuffer(fb, work, w, h)
        ctx.copy_framebuffer(fb, other, w, h)
        ctx.synchronize()
        t0 = time.perf_counter()
        stats = z.despeckle(work, w, h, (work,))
        t1 = time.perf_counter()
        m1, a1 = z.despeckle_time_ms()
        ctx.copy_framebuffer(fb, work, w, h)
        ctx.synchronize()
        z.despeckle(work, w, h, (work, other))
        m2, a2 = z.despeckle_time_ms()
        t0c = time.perf_counter()
        for _ in range(COPIES):
            ctx.copy_framebuffer(fb, other, w, h)
        ctx.synchronize()
        t1c = time.perf_counter()
        if r >= WARM:
            t["measure"] += [m1, m2]; t["apply1"].append(a1); t["apply2"].append(a2); t["call1"].append((t1 - t0) * 1e3); t["copy"].append((t1c - t0c) * 1e3 / COPIES)
    z.close()
    ctx.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    show = lambda k: f"{med[k]:.4f} ms (min {min(t[k]):.4f}, max {max(t[k]):.4f})"
    return [f"cfg2_hdr {w}x{h}, 4 passes: {stats['clamped']} of {w * h} pixels clamped ({100.0 * stats['clamped'] / (w * h):.3f} %), {stats['bad']} bad; the defaults; "
            f"{ROUNDS} rounds behind {WARM} warm-up rounds",
            f"  measure                    : {show('measure')} = {med['measure'] / med['copy']:.2f} x the copy; {12.0 * w * h / med['measure'] / 1e6:.0f} GB/s of guide read",
            f"  apply, one frame           : {show('apply1')} = {med['apply1'] / med['copy']:.2f} x the copy",
            f"  apply, two frames          : {show('apply2')}",
            f"  crh_framebuffer_copy       : {show('copy')} ({COPIES} back to back, wall / {COPIES}); {24.0 * w * h / med['copy'] / 1e6:.0f} GB/s read + written",
            f"  whole call, one frame, wall: {show('call1')}"]


def measure_pictures(api, name, w, h):
    ctx = api.Context(0)
    ctx.upload(api.Scene(blob(name)))
    bounces = SCENES[name]
    ref, fb, half, work, work_half, out = (ctx.framebuffer(w, h) for _ in range(6))
    aov = ctx.aov_buffer(w, h)
    ctx.render_region(ref, w, h, 256, bounces)
    want = ctx.download(ref, w, h)
    lines = [f"{name} {w}x{h} against its 256-pass frame (RMSE: linear / of x / (1 + x)); the defaults 2, 4, 4, 2^-6"]
    for n in (16, 64):
        ctx.render_region(fb, w, h, n, bounces, first_pass=0, pass_count=n // 2)
        ctx.copy_framebuffer(fb, half, w, h)
        ctx.render_region(fb, w, h, n, bounces, first_pass=n // 2, pass_count=n - n // 2)
        ctx.render_aov(aov, w, h, n, pass_count=min(16, n))
        frame = ctx.download(fb, w, h)
        ctx.copy_framebuffer(fb, work, w, h)
        ctx.copy_framebuffer(half, work_half, w, h)
        stats = ctx.despeckle(work, w, h, also=(work_half,))
        clean = ctx.download(work, w, h)
        removed = 1.0 - lum(clean).sum() / lum(frame).sum()
        rows = {"the frame": rmse2(frame, want), "the despeckled frame": rmse2(clean, want)}
        ctx.denoise(fb, aov, w, h, out=out)
        rows["denoise"] = rmse2(ctx.download(out, w, h), want)
        ctx.denoise(work, aov, w, h, out=out)
        rows["despeckle + denoise"] = rmse2(ctx.download(out, w, h), want)
        ctx.denoise_variance(fb, half, aov, w, h, n // 2, n, out=out)
        rows["denoise_variance"] = rmse2(ctx.download(out, w, h), want)
        ctx.denoise_variance(work, work_half, aov, w, h, n // 2, n, out=out)
        rows["despeckle + denoise_variance"] = rmse2(ctx.download(out, w, h), want)
        lines.append(f"  {n:3d} passes: {stats['clamped']} pixels clamped ({100.0 * stats['clamped'] / (w * h):.3f} %), {stats['bad']} bad, {100.0 * removed:.3f} % of the luminance removed, "
                     f"brightest clamped {float(stats['max_clamped']):.4g}, smallest scale {float(stats['min_scale']):.4g}")
        for what, (lin, comp) in rows.items():
            lines.append(f"      {what:30s}: {lin:10.5f} / {comp:.5f}")
    ctx.close()
    return lines


def measure_defaults(api, w, h):
    lines = [f"the defaults on 4-pass frames at {w}x{h}:"]
    for name in SCENES:
        if not blob(name):
            lines.append(f"  {name}: scenes/_built/{name}.blob is not built")
            continue
        ctx = api.Context(0)
        ctx.upload(api.Scene(blob(name)))
        fb = ctx.framebuffer(w, h)
        ctx.render_region(fb, w, h, 4, SCENES[name])
        frame = ctx.download(fb, w, h)
        stats = ctx.despeckle(fb, w, h)
        removed = 1.0 - lum(ctx.download(fb, w, h)).sum() / lum(frame).sum()
        lines.append(f"  {name:13s}: {100.0 * stats['clamped'] / (w * h):.3f} % of the pixels clamped, {100.0 * removed:.3f} % of the luminance removed, {stats['bad']} bad")
        ctx.close()
    return lines


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return args[args.index(name) + 1] if name in args else default
    sys.path.insert(0, REPO)
    from __graft_entry__ import load_package
    api = load_package().api
    out = opt("--out", os.path.join(REPO, "profiles", "despeckle_rate.log"))
    sizes = [tuple(int(v) for v in s.split("x")) for s in opt("--sizes", "1280x720,3840x2160").split(",")]
    pw, ph = (int(v) for v in opt("--picture-size", "1280x720").split("x"))
    if api.device_count() < 1:
        lines = ["no HIP device here: nothing is measured"]
    elif not blob("cfg2_hdr"):
        lines = ["scenes/_built/cfg2_hdr.blob is not built (it needs the reference's assets at build time): nothing is measured"]
    else:
        import cray_amd.exrzip as exrzip
        lines = []
        for w, h in sizes:
            lines += measure_time(api, exrzip, w, h)
        for name in ("cfg2_hdr", "cfg3_venus"):
            lines += measure_pictures(api, name, pw, ph) if blob(name) else [f"scenes/_built/{name}.blob is not built"]
        lines += measure_defaults(api, pw, ph)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
