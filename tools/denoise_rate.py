#!/usr/bin/env python3
"""denoise_rate.py — what crh_denoise costs, against producing its guides, and which form of the iteration kernel each step should use.

    python tools/denoise_rate.py [--forms-lib PATH] [--runs 2] [--no-regs] [--no-measure] [--append] [--out profiles/denoise_rate.log]

The workload: BASELINE configs[1] (the cfg2 blob bench.py uses) at 1280 x 720, 16 passes of 16 of the frame and 16 passes of guides.
  product   this tree's library: crh_denoise with the defaults (5 iterations), timed by crh_denoise_time_ms — the median of 10 calls after a warm-up call — and
            launch by launch (crh_debug_denoise_launch_ms, medians of the same calls); in the same process the yardstick, k_aov at 16 passes, timed by
            crh_aov_kernel_time_ms with the method of tools/aov_rate.py (one warm-up dispatch, the best of three). The whole denoise may take no longer than
            the guides took: a consumer that costs more than producing its input is the wrong shape.
  forms     --forms-lib (default c-ray_amd/_lib/variants/denoise_forms.so: this tree built with -DCRH_DENOISE_ALL_FORMS, which also holds the dense LDS tiles of
            the steps 2, 4, 8): the same calls with CRH_DENOISE_FORM forcing every step to the direct gather (d), the dense tile (t; none at step 16: 221 KB) and
            the sub-lattice tile (l); the outputs of the three must be the same bits. The per-step medians are the A/B behind dnDefaultForm (cray_hip.hip).
Each run is a process of its own (one library per process); the two kinds alternate, --runs times each, and the log quotes the best run's medians. The log also
holds tools/kernel_regs.py's lines for the denoise kernels (with -DCRH_DENOISE_ALL_FORMS: every form).
"""
import hashlib
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PASSES, BOUNCES, ITERATIONS, CALLS, AOV_REPS = 1280, 720, 16, 8, 5, 10, 3
FORMS = {"direct": "ddddd", "dense": "ttttd", "sub-lattice": "lllll"}


def blob_path():
    for name in ("cfg2_hdr", "cfg2_hdr_envstandin"):
        p = os.path.join(REPO, "scenes", "_built", name + ".blob")
        if os.path.exists(p):
            return p
    raise SystemExit("scenes/_built/cfg2_hdr.blob (or its stand-in) is not built: run __graft_entry__.build()")


def child(kind):
    """One process, one library (CRH_LIB): the frame and the guides once, then the timed calls."""
    sys.path.insert(0, REPO)
    from __graft_entry__ import load_package
    api = load_package().api
    ctx = api.Context(0)
    ctx.upload(api.Scene(blob_path()))
    fb, out, buf = ctx.framebuffer(W, H), ctx.framebuffer(W, H), ctx.aov_buffer(W, H)
    ctx.render_region(fb, W, H, PASSES, BOUNCES)
    rec = {}
    if kind == "product":
        times = []
        for _ in range(AOV_REPS + 1):          # the first dispatch warms the kernel up
            ctx.clear_aov(buf, W, H)
            ctx.render_aov(buf, W, H, PASSES)
            times.append(ctx.aov_kernel_time_ms())
        rec["aov_ms"], rec["aov_all_ms"] = min(times[1:]), times
        configs = {"default": None}
    else:
        ctx.render_aov(buf, W, H, PASSES)
        configs = FORMS
    for name, forms in configs.items():
        if forms is None:
            os.environ.pop("CRH_DENOISE_FORM", None)
        else:
            os.environ["CRH_DENOISE_FORM"] = forms
        total, launches = [], []
        for _ in range(CALLS + 1):             # the first call warms the kernels up (and sizes the scratch)
            ctx.denoise(fb, buf, W, H, out=out, iterations=ITERATIONS)
            total.append(ctx.denoise_time_ms())
            launches.append(ctx.denoise_launch_ms())
        img = ctx.download(out, W, H)
        rec[name] = {"ms": statistics.median(total[1:]), "min_ms": min(total[1:]), "max_ms": max(total[1:]), "warmup_ms": total[0],
                     "launch_ms": [statistics.median(l[k] for l in launches[1:]) for k in range(ITERATIONS + 1)],
                     "md5": hashlib.md5(img.tobytes()).hexdigest(), "finite": bool((img == img).all()), "mean": float(img.mean())}
    ctx.close()
    print("RATE " + json.dumps(rec), flush=True)


def main():
    args = sys.argv[1:]
    if os.environ.get("DENOISE_RATE_CHILD"):
        return child(os.environ["DENOISE_RATE_CHILD"])

    def opt(name, default):
        return args[args.index(name) + 1] if name in args else default
    forms_lib = os.path.abspath(opt("--forms-lib", os.path.join(REPO, "c-ray_amd", "_lib", "variants", "denoise_forms.so")))
    runs = int(opt("--runs", "2"))
    out = opt("--out", os.path.join(REPO, "profiles", "denoise_rate.log"))
    lines = []
    if "--no-measure" not in args:
        if not os.path.exists(forms_lib):
            raise SystemExit(f"{forms_lib} is missing: build this tree's library there with -DCRH_DENOISE_ALL_FORMS (c-ray_amd/build.py prints the command)")
        res = {"product": [], "forms": []}
        for r in range(runs):
            for kind in ("product", "forms"):
                env = dict(os.environ, DENOISE_RATE_CHILD=kind)
                env.pop("CRH_DENOISE_FORM", None)
                if kind == "forms":
                    env["CRH_LIB"] = forms_lib
                p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
                got = [l for l in p.stdout.splitlines() if l.startswith("RATE ")]
                if p.returncode != 0 or not got:
                    raise SystemExit(f"{kind} run {r} failed (rc {p.returncode}):\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")          # nothing more is started on the GPU
                rec = json.loads(got[0][5:])
                res[kind].append(rec)
                for name, d in rec.items():
                    if isinstance(d, dict):
                        lines.append(f"run {r} {kind:8s} {name:12s} median {d['ms']:7.3f} ms of {CALLS} calls (min {d['min_ms']:.3f}, max {d['max_ms']:.3f}; warm-up {d['warmup_ms']:.3f})   "
                                     f"prepare {d['launch_ms'][0]:.3f} | steps " + " ".join(f"{t:.3f}" for t in d["launch_ms"][1:]) + f"   md5 {d['md5'][:12]}")
                if "aov_ms" in rec:
                    lines.append(f"run {r} {kind:8s} k_aov        best   {rec['aov_ms']:7.3f} ms (timed dispatches: {', '.join('%.3f' % t for t in rec['aov_all_ms'][1:])}; warm-up {rec['aov_all_ms'][0]:.3f})")
        lines.insert(0, f"{os.path.basename(blob_path())} {W}x{H}: frame {PASSES} passes of {PASSES}, {BOUNCES} bounces; guides {PASSES} passes; crh_denoise, {ITERATIONS} iterations, the default sigmas")
        best = min(res["product"], key=lambda rec: rec["default"]["ms"])
        d, a = best["default"], min(rec["aov_ms"] for rec in res["product"])
        lines.append(f"crh_denoise_time_ms, {ITERATIONS} iterations (product library)   median {d['ms']:7.3f} ms   = prepare {d['launch_ms'][0]:.3f} + steps 1, 2, 4, 8, 16: "
                     + " + ".join(f"{t:.3f}" for t in d["launch_ms"][1:]))
        lines.append(f"crh_aov_kernel_time_ms, {PASSES} passes (k_aov, the yardstick) best   {a:7.3f} ms")
        lines.append(f"ratio denoise / guides = {d['ms'] / a:.3f}   (bound 1.0: {'met' if d['ms'] <= a else 'MISSED'})")
        pixels = W * H
        lines.append(f"per step: {pixels} pixels x 25 taps x 32 B = {pixels * 25 * 32 / 1e6:.0f} MB of tap reads, 5 correctly rounded divisions a tap")
        lines.append("A/B per step (forms library; median of the launch's times, ms; the best of the runs):")
        lines.append("  step   direct    dense  sub-lattice   fastest")
        table = {name: [min(rec[name]["launch_ms"][1 + i] for rec in res["forms"]) for i in range(ITERATIONS)] for name in FORMS}
        for i in range(ITERATIONS):
            row = {name: table[name][i] for name in FORMS if not (name == "dense" and FORMS[name][i] != "t")}
            win = min(row, key=row.get)
            lines.append(f"  {1 << i:4d}  " + "  ".join(f"{row[name]:7.3f}" if name in row else "      -" for name in FORMS) + f"      {win}")
        md5s = {rec[name]["md5"] for rec in res["forms"] for name in FORMS} | {rec["default"]["md5"] for rec in res["product"]}
        fine = all(rec[name]["finite"] for rec in res["forms"] for name in FORMS)
        lines.append(f"outputs of all forms and of the product library: {'bit-identical' if len(md5s) == 1 else 'DIFFERENT: ' + ', '.join(sorted(md5s))}, {'finite' if fine else 'NOT FINITE'}")
    if "--no-regs" not in args:
        regs = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), "--filter", "k_denoise", "-DCRH_DENOISE_ALL_FORMS"], capture_output=True, text=True)
        lines += [l for l in regs.stdout.splitlines() if l.strip()] or [f"tools/kernel_regs.py failed: {regs.stderr[-300:]}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a" if "--append" in args else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
