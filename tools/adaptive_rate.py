#!/usr/bin/env python3
"""adaptive_rate.py — what the adaptive step costs, and what adaptive sampling buys on the bench scene.

    python tools/adaptive_rate.py [--cells] [--no-regs] [--no-measure] [--append] [--out profiles/adaptive_rate.log]

The workload: BASELINE configs[1] (the cfg2 blob bench.py uses) at 1280 x 720, 8 bounces, 64 x 64 tiles (the scene file's own: 20 x 12 = 240), cap 256 of 256.
One process:
  step      the frame after passes [0, 8), crh_framebuffer_copy, passes [8, 16). Then, alternating, 20 timed calls each after a warm-up call each:
            crh_adaptive_step over the full tile list at threshold 0 — every tile is measured and copied, the step's most expensive case — timed by
            crh_adaptive_time_ms (events around the kernel), and crh_framebuffer_copy of the same frame: 50 copies queued back to back, by the host clock
            around 51 copies + synchronize minus the same around 1 copy + synchronize (a device-to-device copy has no entry that times it).
            The log quotes medians. Condition: step <= 3 x copy — the step moves at most 36 bytes a pixel against the copy's 24 (1.5 x) and gets a factor 2
            for the reduction and its barriers.
  loop      the uniform frames at 32, 64, 128 and 256 passes (wall time of render + synchronize, rays), then crh_render_adaptive with min_passes 16 at the
            thresholds 0.2, 0.1, 0.05, 0.025: rays, wall time of the whole loop, the histogram of pass counts and the RMSE against the uniform 256-pass frame.
            Every figure is one run behind a warm-up render; no number is promised.
--cells adds the cell-granular step and loop (crh_adaptive_step_cells, crh_render_adaptive_cells), everything re-taken in the same run:
  step      in the same alternation, crh_adaptive_step_cells (cells of 16, threshold 0, dilate 1) over the same list on the same input, by crh_adaptive_time_ms.
            Condition: cell step <= 1.5 x the rectangle step of this run — the same 36 bytes a pixel, two barriers instead of eight, sixteen cells
            serialised over four waves, and the two events' couple of microseconds.
  loop      behind the rectangle-granular rows, crh_render_adaptive_cells at cells of 32, 16 and 8, the same thresholds, dilate 0 and 1: rays, wall time of the
            whole loop, RMSE against the uniform 256-pass frame, cells by pass count. Every adaptive row (the rectangle-granular ones too) is then set against
            the uniform frame twice: against the cheapest uniform frame measured in this run whose RMSE is equal or lower (a coarse yardstick: there are four),
            and against the uniform frame of EQUAL RMSE. The latter is a model, stated here: the uniform n-pass frame is the mean of the first n of the
            reference's 256 passes, so its RMSE against the reference is sigma sqrt(1 / n - 1 / 256); sigma is fitted to the measured uniform rows (the log
            prints each row's own sigma: they agree to a percent), n follows from the row's RMSE, and the wall time of n uniform passes is interpolated
            linearly between the measured uniform frames.
The log also holds tools/kernel_regs.py's lines for k_adaptive_step and the render kernels (--no-measure: only those; that is what a machine without a GPU
can write).
"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, CAP, BOUNCES, TILE, MIN_PASSES, CALLS, COPIES = 1280, 720, 256, 8, 64, 16, 20, 50
THRESHOLDS = (0.2, 0.1, 0.05, 0.025)
UNIFORM = (32, 64, 128)
CELLS = (32, 16, 8)
STEP_CELL = 16


def rmse(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()))


def measure(cells=False):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from __graft_entry__ import load_package
    from denoise_rate import blob_path
    pkg = load_package()
    api = pkg.api
    ctx = api.Context(0)
    ctx.set_option(pkg.abi.OPT_COUNTER_LEVEL, 1)          # paths and rays only, as in a timed run
    ctx.upload(api.Scene(blob_path()))
    tiles = pkg.tiles.quantize_image(W, H, TILE, TILE, pkg.tiles.ORDER_NORMAL)
    fb, half, scratch = ctx.framebuffer(W, H), ctx.framebuffer(W, H), ctx.framebuffer(W, H)
    lines = [f"{os.path.basename(blob_path())} {W}x{H}, {BOUNCES} bounces, {len(tiles)} tiles of {TILE} x {TILE}, min_passes {MIN_PASSES}, cap {CAP} of {CAP}"]

    # ---- the step against the copy ----
    ctx.render_tiles(fb, W, H, CAP, BOUNCES, tiles, first_pass=0, pass_count=8)
    ctx.copy_framebuffer(fb, half, W, H)
    ctx.render_tiles(fb, W, H, CAP, BOUNCES, tiles, first_pass=8, pass_count=8)
    ctx.synchronize()

    def copies_ms(n):
        """n copies queued back to back, then one synchronize: the host clock around them."""
        ctx.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            ctx.copy_framebuffer(fb, scratch, W, H)
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3
    step, measure_only, copy, cell_step = [], [], [], []
    for i in range(CALLS + 1):          # the first round warms everything up
        ctx.copy_framebuffer(half, scratch, W, H)          # the step at threshold 0 overwrites half: every timed step sees the same input
        ctx.synchronize()
        _, flags = ctx.adaptive_step(fb, scratch, W, H, tiles, 0.0)
        step.append((ctx.adaptive_time_ms(), int(flags.sum())))
        ctx.adaptive_step(fb, scratch, W, H, tiles, float("inf"))
        measure_only.append(ctx.adaptive_time_ms())
        copy.append((copies_ms(COPIES + 1) - copies_ms(1)) / COPIES)          # (the difference leaves the launch and the synchronize of a single call out)
        if cells:
            ctx.copy_framebuffer(half, scratch, W, H)
            ctx.synchronize()
            _, flags = ctx.adaptive_step_cells(fb, scratch, W, H, tiles, STEP_CELL, 0.0, dilate=1)
            cell_step.append((ctx.adaptive_time_ms(), int(flags.sum()), len(flags)))
    s, m, c = statistics.median(t for t, _ in step[1:]), statistics.median(measure_only[1:]), statistics.median(copy[1:])
    lines.append(f"crh_adaptive_step, threshold 0 ({step[-1][1]} of {len(tiles)} tiles copied): kernel median {s:.4f} ms (min {min(t for t, _ in step[1:]):.4f}, warm-up {step[0][0]:.4f}); "
                 f"measure only (threshold inf): {m:.4f} ms")
    lines.append(f"crh_framebuffer_copy of the same frame, per copy of {COPIES} queued back to back (host clock, {COPIES + 1} copies + synchronize minus 1 copy + synchronize): "
                 f"median {c:.4f} ms (min {min(copy[1:]):.4f})")
    lines.append(f"ratio step / copy = {s / c if c > 0 else float('nan'):.2f}   (condition 3.0: {'met' if c > 0 and s <= 3 * c else 'MISSED'})")

    if cells:
        k = statistics.median(t for t, _, _ in cell_step[1:])
        lines.append(f"crh_adaptive_step_cells, cells of {STEP_CELL}, threshold 0, dilate 1 ({cell_step[-1][1]} of {cell_step[-1][2]} cells copied), alternating with the above: "
                     f"kernel median {k:.4f} ms (min {min(t for t, _, _ in cell_step[1:]):.4f}, warm-up {cell_step[0][0]:.4f})")
        lines.append(f"ratio cell step / rectangle step = {k / s if s > 0 else float('nan'):.2f}   (condition 1.5: {'met' if s > 0 and k <= 1.5 * s else 'MISSED'})")

    # ---- the loop against uniform frames ----
    def timed(render):
        ctx.clear(fb, W, H)
        ctx.clear(half, W, H)
        ctx.reset_counters()
        ctx.synchronize()
        t = time.perf_counter()
        out = render()
        ctx.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        return out, ms, ctx.counters()["rays"], ctx.download(fb, W, H)
    timed(lambda: ctx.render_tiles(fb, W, H, CAP, BOUNCES, tiles, first_pass=0, pass_count=MIN_PASSES))          # warm-up
    _, ms, rays, reference = timed(lambda: ctx.render_tiles(fb, W, H, CAP, BOUNCES, tiles, first_pass=0, pass_count=CAP))
    uniform = [(ms, 0.0, f"uniform {CAP}")]          # (wall ms, rmse, name) of every uniform frame of this run
    wall = {0: 0.0, CAP: ms}                            # wall ms of n uniform passes
    sigmas = []
    lines.append(f"uniform {CAP:3d} passes: {rays:11d} rays {ms:9.2f} ms   (the reference of the RMSE column)")
    for n in UNIFORM:
        _, ms, rays, frame = timed(lambda: ctx.render_tiles(fb, W, H, CAP, BOUNCES, tiles, first_pass=0, pass_count=n))
        lines.append(f"uniform {n:3d} passes: {rays:11d} rays {ms:9.2f} ms   rmse {rmse(frame, reference):.6f}")
        uniform.append((ms, rmse(frame, reference), f"uniform {n}"))
        wall[n] = ms
        sigmas.append(rmse(frame, reference) / (1.0 / n - 1.0 / CAP) ** 0.5)
    sigma = sum(sigmas) / len(sigmas)

    def against_uniform(ms, e):
        """(the verdict's text, beats a measured uniform frame, beats the uniform frame of equal RMSE)"""
        rival = min((u for u in uniform if u[1] <= e), key=lambda u: u[0])
        n = 1.0 / ((e / sigma) ** 2 + 1.0 / CAP)
        known = sorted(wall)
        lo = max(k for k in known if k <= n)
        hi = min(k for k in known if k >= n)
        equal = wall[lo] if hi == lo else wall[lo] + (wall[hi] - wall[lo]) * (n - lo) / (hi - lo)
        return (f"{'beats' if ms < rival[0] else 'loses to'} {rival[2]} ({rival[0]:.2f} ms, rmse {rival[1]:.6f}); uniform at equal rmse: {n:5.1f} passes, {equal:6.2f} ms: "
                f"{'BEATS it' if ms < equal else 'loses'}"), ms < rival[0], ms < equal
    if cells:
        lines.append(f"uniform rmse model sigma sqrt(1 / n - 1 / {CAP}): sigma per measured row {', '.join(f'{x:.4f}' for x in sigmas)}; used {sigma:.4f}")
    for threshold in THRESHOLDS:
        (passes, errors), ms, rays, frame = timed(lambda: ctx.render_adaptive(fb, half, W, H, CAP, BOUNCES, tiles, min_passes=MIN_PASSES, threshold=threshold))
        hist = ", ".join(f"{n}: {int((passes == n).sum())}" for n in sorted(set(passes.tolist())))
        lines.append(f"adaptive {threshold:5.3f}:      {rays:11d} rays {ms:9.2f} ms   rmse {rmse(frame, reference):.6f}   mean passes {passes.mean():6.1f}   tiles by pass count {{{hist}}}   "
                     f"largest error left {errors.max():.4f}" + (f"   {against_uniform(ms, rmse(frame, reference))[0]}" if cells else ""))
    if cells:
        beaten, equalled, rows = [], [], 0
        for cell in CELLS:
            for dilate in (0, 1):
                for threshold in THRESHOLDS:
                    (passes, errors), ms, rays, frame = timed(lambda: ctx.render_adaptive_cells(fb, half, W, H, CAP, BOUNCES, tiles, min_passes=MIN_PASSES, threshold=threshold,
                                                                                                cell=cell, dilate=dilate))
                    e = rmse(frame, reference)
                    hist = ", ".join(f"{n}: {int((passes == n).sum())}" for n in sorted(set(passes.tolist())))
                    verdict, measured, equal = against_uniform(ms, e)
                    rows += 1
                    if measured:
                        beaten.append(f"cells {cell} dilate {dilate} threshold {threshold}")
                    if equal:
                        equalled.append(f"cells {cell} dilate {dilate} threshold {threshold}")
                    lines.append(f"cells {cell:2d} dilate {dilate} {threshold:5.3f}: {rays:11d} rays {ms:9.2f} ms   rmse {e:.6f}   mean passes {passes.mean():6.1f}   cells by pass count {{{hist}}}   "
                                 f"largest error left {errors.max():.4f}   {verdict}")
        lines.append(f"cell-granular rows that beat, in wall time, the cheapest uniform frame of equal or lower RMSE of this run: {len(beaten)} of {rows}" +
                     (": " + "; ".join(beaten) if beaten else ""))
        lines.append(f"cell-granular rows that beat, in wall time, the uniform frame of equal RMSE (the model above): {len(equalled)} of {rows}" + (": " + "; ".join(equalled) if equalled else ""))
    ctx.close()
    return lines


def main():
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(REPO, "profiles", "adaptive_rate.log")
    lines = [] if "--no-measure" in args else measure("--cells" in args)
    if "--no-regs" not in args:
        regs = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py")], capture_output=True, text=True)
        lines += [l for l in regs.stdout.splitlines() if "k_adaptive" in l or "k_pathtrace_roll" in l] or [f"tools/kernel_regs.py failed: {regs.stderr[-300:]}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a" if "--append" in args else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
