#!/usr/bin/env python3
"""denoise_variance_rate.py — what crh_denoise_variance costs against the plain crh_denoise of the same run, and against producing the guides.

    python tools/denoise_variance_rate.py [--no-regs] [--no-measure] [--append] [--out profiles/denoise_variance_rate.log]

The workload is tools/denoise_rate.py's: BASELINE configs[1] (the cfg2 blob bench.py uses) at 1280 x 720, 16 passes of 16 of the frame — here as passes [0, 8),
crh_framebuffer_copy, passes [8, 16) — and 16 passes of guides; 5 iterations, each filter's default sigmas. One process: k_aov at 16 passes with the method of
tools/aov_rate.py (one warm-up dispatch, the best of three), then the two filters in alternation, 10 timed calls each after a warm-up call each (which also sizes
the scratch), timed by crh_denoise_time_ms and launch by launch (crh_debug_denoise_launch_ms); the log quotes medians.
Two conditions: the variance-guided filter takes at most 1.5 x the plain one's time, and — the denoiser's own bound — no longer than the guides took.
The log also holds tools/kernel_regs.py's lines for the denoise kernels.
"""
import hashlib
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PASSES, BOUNCES, ITERATIONS, CALLS, AOV_REPS = 1280, 720, 16, 8, 5, 10, 3


def measure():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from __graft_entry__ import load_package
    from denoise_rate import blob_path
    api = load_package().api
    ctx = api.Context(0)
    ctx.upload(api.Scene(blob_path()))
    fb, half, out, buf = ctx.framebuffer(W, H), ctx.framebuffer(W, H), ctx.framebuffer(W, H), ctx.aov_buffer(W, H)
    ctx.render_region(fb, W, H, PASSES, BOUNCES, first_pass=0, pass_count=PASSES // 2)
    ctx.copy_framebuffer(fb, half, W, H)
    ctx.render_region(fb, W, H, PASSES, BOUNCES, first_pass=PASSES // 2, pass_count=PASSES - PASSES // 2)
    aov = []
    for _ in range(AOV_REPS + 1):          # the first dispatch warms the kernel up
        ctx.clear_aov(buf, W, H)
        ctx.render_aov(buf, W, H, PASSES)
        aov.append(ctx.aov_kernel_time_ms())
    calls = {"plain": lambda: ctx.denoise(fb, buf, W, H, out=out, iterations=ITERATIONS),
             "variance": lambda: ctx.denoise_variance(fb, half, buf, W, H, PASSES // 2, PASSES, out=out, iterations=ITERATIONS)}
    total, launches, md5 = {k: [] for k in calls}, {k: [] for k in calls}, {}
    for i in range(CALLS + 1):             # the first call of each kind warms its kernels up
        for kind, call in calls.items():
            call()
            total[kind].append(ctx.denoise_time_ms())
            launches[kind].append(ctx.denoise_launch_ms())
            if i == CALLS:
                img = ctx.download(out, W, H)
                md5[kind] = (hashlib.md5(img.tobytes()).hexdigest()[:12], bool((img == img).all()))
    ctx.close()
    lines = [f"{os.path.basename(blob_path())} {W}x{H}: frame {PASSES} passes of {PASSES} ({PASSES // 2} + copy + {PASSES - PASSES // 2}), {BOUNCES} bounces; guides {PASSES} passes; "
             f"{ITERATIONS} iterations, the default sigmas; the two filters alternate, {CALLS} timed calls each"]
    med = {}
    for kind in calls:
        t, per = total[kind][1:], launches[kind][1:]
        med[kind] = statistics.median(t)
        steps = [statistics.median(l[k] for l in per) for k in range(len(per[0]))]
        names = "prepare, steps 1, 2, 4, 8, 16" if kind == "plain" else "prepare, prefilter, steps 1, 2, 4, 8, 16"
        lines.append(f"{'crh_denoise' if kind == 'plain' else 'crh_denoise_variance':22s} median {med[kind]:7.3f} ms (min {min(t):.3f}, max {max(t):.3f}; warm-up {total[kind][0]:.3f})   "
                     f"{names}: " + " ".join(f"{s:.3f}" for s in steps) + f"   md5 {md5[kind][0]} {'finite' if md5[kind][1] else 'NOT FINITE'}")
    a = min(aov[1:])
    lines.append(f"crh_aov_kernel_time_ms, {PASSES} passes (k_aov, the yardstick) best {a:7.3f} ms (timed dispatches: {', '.join('%.3f' % t for t in aov[1:])}; warm-up {aov[0]:.3f})")
    ratio = med["variance"] / med["plain"]
    lines.append(f"ratio variance-guided / plain = {ratio:.3f}   (bound 1.5: {'met' if ratio <= 1.5 else 'MISSED'})")
    lines.append(f"ratio variance-guided / guides = {med['variance'] / a:.3f}   (bound 1.0: {'met' if med['variance'] <= a else 'MISSED'})")
    return lines


def main():
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(REPO, "profiles", "denoise_variance_rate.log")
    lines = [] if "--no-measure" in args else measure()
    if "--no-regs" not in args:
        regs = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), "--filter", "k_denoise"], capture_output=True, text=True)
        lines += [l for l in regs.stdout.splitlines() if l.strip()] or [f"tools/kernel_regs.py failed: {regs.stderr[-300:]}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a" if "--append" in args else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
