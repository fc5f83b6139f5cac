#!/usr/bin/env python3
"""aov_rate.py — what crh_render_aov costs: k_aov against the render kernel on the same primary rays.

    python tools/aov_rate.py [--baseline-lib PATH] [--runs 3] [--no-regs] [--no-measure] [--out profiles/aov_rate.log]

The workload: BASELINE configs[1] (the cfg2 blob bench.py uses) at 1280 x 720, 16 passes of 16.
  aov       this tree's library, Context.render_aov, timed by crh_aov_kernel_time_ms
  baseline  --baseline-lib (default c-ray_amd/_lib/variants/parent.so: the library of the commit before the AOV entry points, which has none of them and is
            therefore bound by hand below), crh_render_region with bounces = 1 over the same 16 passes, counter level 1, timed by crh_kernel_time_ms: the same
            camera rays and first hits, one bsdf sample more per path, inside the tuned wave machine
Each run is a process of its own (one library per process) that warms its kernel up with one untimed dispatch and reports the best of three timed ones; the
two kinds alternate, --runs times each. The AOV dispatch may take at most 1.5 x the baseline (the one-ray-per-lane walk, the 32-byte pixel and both branches
of a mix are allowed for; a kernel that fell into scratch or lost its occupancy is not). The log also holds tools/kernel_regs.py's lines for k_aov.
"""
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PASSES, REPS = 1280, 720, 16, 3


def blob_path():
    for name in ("cfg2_hdr", "cfg2_hdr_envstandin"):
        p = os.path.join(REPO, "scenes", "_built", name + ".blob")
        if os.path.exists(p):
            return p
    raise SystemExit("scenes/_built/cfg2_hdr.blob (or its stand-in) is not built: run __graft_entry__.build()")


def child_aov():
    sys.path.insert(0, REPO)
    from __graft_entry__ import load_package
    api = load_package().api
    ctx = api.Context(0)
    ctx.upload(api.Scene(blob_path()))
    buf = ctx.aov_buffer(W, H)
    times = []
    for i in range(REPS + 1):          # the first dispatch warms the kernel up
        ctx.clear_aov(buf, W, H)
        ctx.render_aov(buf, W, H, PASSES)
        times.append(ctx.aov_kernel_time_ms())
    cover = float(ctx.download_aov(buf, W, H)[..., 7].mean())
    ctx.close()
    print("RATE " + json.dumps({"ms": min(times[1:]), "all_ms": times, "coverage": cover}), flush=True)


def child_baseline(lib):
    """crh_render_region of a library that may predate crh_render_aov: only the entry points this needs are bound."""
    sys.path.insert(0, REPO)
    from __graft_entry__ import load_package
    abi = load_package().abi
    try:
        import torch  # noqa: F401  (its HIP runtime first, as api.library() does)
    except Exception:
        pass
    L = C.CDLL(lib)
    ctx, fb = C.c_void_p(), C.c_void_p()
    scene, prefs = C.POINTER(abi.SceneDesc)(), abi.BlobPrefs()
    L.crh_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int64]
    L.crh_last_error.restype = C.c_char_p

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"{what} failed with {rc}: {(L.crh_last_error() or b'').decode()}")
    ok(L.crh_context_create(0, None, C.byref(ctx)), "crh_context_create")
    ok(L.crh_set_option(ctx, abi.OPT_COUNTER_LEVEL, 1), "crh_set_option")
    ok(L.crh_blob_load(os.fsencode(blob_path()), C.byref(scene), C.byref(prefs)), "crh_blob_load")
    ok(L.crh_scene_upload(ctx, scene), "crh_scene_upload")
    ok(L.crh_framebuffer_alloc(ctx, W, H, C.byref(fb)), "crh_framebuffer_alloc")
    p = abi.RenderParams(0, 0, W, H, W, H, 0, PASSES, PASSES, 1)
    times = []
    for i in range(REPS + 1):
        ok(L.crh_framebuffer_clear(ctx, fb, W, H), "crh_framebuffer_clear")
        ok(L.crh_render_region(ctx, C.byref(p), fb), "crh_render_region")
        ok(L.crh_synchronize(ctx), "crh_synchronize")
        ms = C.c_float()
        ok(L.crh_kernel_time_ms(ctx, C.byref(ms), None, None), "crh_kernel_time_ms")
        times.append(ms.value)
    L.crh_last_kernel_name.restype = C.c_char_p
    L.crh_last_kernel_name.argtypes = [C.c_void_p]
    name = (L.crh_last_kernel_name(ctx) or b"").decode()
    L.crh_context_destroy(ctx)
    print("RATE " + json.dumps({"ms": min(times[1:]), "all_ms": times, "kernel": name}), flush=True)


def main():
    args = sys.argv[1:]
    if os.environ.get("AOV_RATE_CHILD") == "aov":
        return child_aov()
    if os.environ.get("AOV_RATE_CHILD") == "baseline":
        return child_baseline(os.environ["AOV_RATE_LIB"])

    def opt(name, default):
        return args[args.index(name) + 1] if name in args else default
    base_lib = os.path.abspath(opt("--baseline-lib", os.path.join(REPO, "c-ray_amd", "_lib", "variants", "parent.so")))
    runs = int(opt("--runs", "3"))
    out = opt("--out", os.path.join(REPO, "profiles", "aov_rate.log"))
    lines = []
    if "--no-measure" not in args:
        if not os.path.exists(base_lib):
            raise SystemExit(f"{base_lib} is missing: build the parent commit's library there")
        res = {"aov": [], "baseline": []}
        for r in range(runs):
            for kind in ("baseline", "aov"):
                env = dict(os.environ, AOV_RATE_CHILD=kind, AOV_RATE_LIB=base_lib)
                p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
                got = [l for l in p.stdout.splitlines() if l.startswith("RATE ")]
                if p.returncode != 0 or not got:
                    raise SystemExit(f"{kind} run {r} failed (rc {p.returncode}):\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")          # nothing more is started on the GPU
                rec = json.loads(got[0][5:])
                res[kind].append(rec)
                lines.append(f"run {r} {kind:8s} {rec['ms']:8.3f} ms   (timed dispatches: {', '.join('%.3f' % t for t in rec['all_ms'][1:])}; warm-up {rec['all_ms'][0]:.3f})"
                             + (f"   {rec['kernel']}" if "kernel" in rec else f"   coverage {rec['coverage']:.4f}"))
        a, b = min(r["ms"] for r in res["aov"]), min(r["ms"] for r in res["baseline"])
        rays = W * H * PASSES
        lines.insert(0, f"{os.path.basename(blob_path())} {W}x{H}, {PASSES} passes of {PASSES} ({rays} camera rays)")
        lines.append(f"crh_render_aov (k_aov)                        best {a:8.3f} ms   {rays / a / 1e3:8.1f} Mrays/s")
        lines.append(f"crh_render_region, bounces = 1 (baseline lib) best {b:8.3f} ms   {rays / b / 1e3:8.1f} Mrays/s")
        lines.append(f"ratio aov / baseline = {a / b:.3f}   (bound 1.5: {'met' if a <= 1.5 * b else 'MISSED'})")
    if "--no-regs" not in args:
        regs = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), "--filter", "k_aov"], capture_output=True, text=True)
        lines += [l for l in regs.stdout.splitlines() if l.strip()] or [f"tools/kernel_regs.py failed: {regs.stderr[-300:]}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a" if "--append" in args else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
