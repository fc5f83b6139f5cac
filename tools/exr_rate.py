#!/usr/bin/env python3
"""exr_rate.py — what the multi-layer OpenEXR output costs on the bench scene (the cfg2 blob bench.py uses) at 1280 x 720 with all 38 channels: the frame, the guides,
a denoised frame and both ranked ID buffers.

    python tools/exr_rate.py [--no-dropin] [--out profiles/exr_rate.log]

One process, behind warm-up rounds, medians of interleaved calls of
  pack      crh_pack_scanlines over the whole frame in one call, its kernel by crh_pack_time_ms (two of the library's events around k_pack_scanlines);
  copy      a device-to-device copy of the same number of bytes — crh_framebuffer_copy of a float buffer of 38 x 1280 x 720 words —, per copy of 20 queued back to
            back, by the host clock around 21 copies + synchronize minus the same around 1 copy + synchronize (the way tools/adaptive_rate.py times it);
  call      the wall time of the whole Context.pack_scanlines call (map upload, kernel, copy through pinned memory, copy out);
  write     the wall time of exr.file_bytes + the file's write to a temporary directory.
The kernel moves the bytes the copy moves but reads them strided; the expectation to confirm or refute is pack <= 2 x copy.
Then the drop-in program on the same frame (256 samples, CRAY_HIP_AOV=16 CRAY_HIP_DENOISE=5) with and without CRAY_HIP_IDS=16 CRAY_HIP_EXR=1: frame_ms of
CRH_DUMP_STATS — all of renderFrame() —, three runs each, alternating, behind one warm-up run.
Without a GPU the log holds tools/kernel_regs.py's line for k_pack_scanlines only, and says so."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PASSES, BOUNCES, GUIDE_PASSES, ROUNDS, WARM, COPIES = 1280, 720, 16, 8, 16, 12, 3, 20


def measure():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from __graft_entry__ import load_package
    from denoise_rate import blob_path
    pkg = load_package()
    api, exr = pkg.api, pkg.exr
    ctx = api.Context(0)
    scene = api.Scene(blob_path())
    ctx.upload(scene)
    fb, dn, aov = ctx.framebuffer(W, H), ctx.framebuffer(W, H), ctx.aov_buffer(W, H)
    bi, bm, ri, rm = (ctx.ids_buffer(W, H) for _ in range(4))          # (the ranked floats [H, W, 6, 2] fit an ID buffer's 16 words a pixel)
    ctx.render_region(fb, W, H, PASSES, BOUNCES)
    ctx.render_aov(aov, W, H, PASSES, pass_count=GUIDE_PASSES)
    ctx.render_ids(bi, bm, W, H, PASSES, pass_count=GUIDE_PASSES)
    ctx.denoise(fb, aov, W, H, out=dn)
    ctx.resolve_ids(bi, W, H, ri)
    ctx.resolve_ids(bm, W, H, rm)
    inst = [f"instance#{i}" for i in range(int(scene.desc.instance_count))]
    mat = [f"material#{i}" for i in range(int(scene.desc.material_count))]
    chans = exr.layer_channels(fb, aov, dn, ri, rm, exr.id_map(inst), exr.id_map(mat))
    strings = dict(exr.crypto_attributes("CryptoObject", inst), **exr.crypto_attributes("CryptoMaterial", mat))
    n = len(chans)
    out_bytes = H * (8 + 4 * n * W)
    big_a, big_b = ctx.framebuffer(n * W, H // 3), ctx.framebuffer(n * W, H // 3)          # 3 x (38 x 1280) x 240 floats: the channels' words
    ctx.synchronize()

    def copies_ms(k):
        ctx.synchronize()
        t = time.perf_counter()
        for _ in range(k):
            ctx.copy_framebuffer(big_a, big_b, n * W, H // 3)
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3
    pack, copy, call, write = [], [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(WARM + ROUNDS):
            t = time.perf_counter()
            blocks = ctx.pack_scanlines([c[1:] for c in chans], W, H)
            t_call = (time.perf_counter() - t) * 1e3
            t_pack = ctx.pack_time_ms()
            t_copy = (copies_ms(COPIES + 1) - copies_ms(1)) / COPIES
            t = time.perf_counter()
            with open(os.path.join(tmp, "layers.exr"), "wb") as f:
                f.write(exr.file_bytes(W, H, [c[0] for c in chans], blocks, strings=strings))
            t_write = (time.perf_counter() - t) * 1e3
            if r >= WARM:
                pack.append(t_pack); copy.append(t_copy); call.append(t_call); write.append(t_write)
    assert len(blocks) == out_bytes
    ctx.close()
    p, c = statistics.median(pack), statistics.median(copy)
    lines = [f"{os.path.basename(blob_path())} {W}x{H}, {n} channels ({len(inst)} instances, {len(mat)} materials), {out_bytes} bytes of pixel data; {ROUNDS} interleaved rounds behind "
             f"{WARM} warm-up rounds, one process, one device"]
    for name, v in (("k_pack_scanlines (crh_pack_time_ms)", pack), (f"device-to-device copy of {4 * n * W * H} bytes", copy), ("Context.pack_scanlines, whole call (wall)", call),
                    ("exr.file_bytes + file write (wall)", write)):
        lines.append(f"{name:46s} median {statistics.median(v):9.4f} ms   min {min(v):9.4f}   max {max(v):9.4f}")
    lines.append(f"kernel: {out_bytes / p / 1e6:.1f} GB/s written (as much read); copy: {4 * n * W * H / c / 1e6:.1f} GB/s")
    lines.append(f"ratio pack / copy = {p / c if c > 0 else float('nan'):.2f}   (expectation 2.0: {'met' if c > 0 and p <= 2 * c else 'MISSED'})")
    return lines


def dropin():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import bench
    exe = os.path.join(REPO, "c-ray_amd", "_lib", "c-ray-hip")
    overlay = os.path.join(REPO, "oracle", "_ref", "input")
    wl = bench.WORKLOADS["cfg2"]
    if not (os.path.exists(exe) and os.path.exists(os.path.join(overlay, wl["scene"]))):
        return ["drop-in program: c-ray-hip or the asset overlay is not built; not measured"]
    import refrun
    both = {"CRAY_HIP_AOV": "16", "CRAY_HIP_DENOISE": "5"}
    kinds = {"without": both, "with CRAY_HIP_IDS=16 CRAY_HIP_EXR=1": dict(both, CRAY_HIP_IDS="16", CRAY_HIP_EXR="1")}
    times = {k: [] for k in kinds}
    size = 0
    for run in range(4):          # the first round warms the machine's file cache and code object cache up
        for kind, extra in kinds.items():
            with tempfile.TemporaryDirectory() as tmp:
                scene = refrun.rewrite_scene(wl["scene"], wl["width"], wl["height"], wl["samples"], wl["bounces"], tile=wl["tile"], out_dir=tmp)
                stats = os.path.join(tmp, "stats.json")
                env = dict(os.environ, CRH_DUMP_STATS=stats, CRAY_HIP_DEVICES="1", **extra)
                for k in ("CRAY_HIP_EXR", "CRAY_HIP_IDS"):
                    if k not in extra:
                        env.pop(k, None)
                proc = subprocess.run([exe], input=json.dumps(scene).encode(), cwd=overlay, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
                if proc.returncode != 0:
                    return [f"drop-in program ({kind}) failed: {proc.stdout.decode(errors='replace')[-300:]}"]
                if run:
                    times[kind].append(json.load(open(stats))["frame_ms"])
                for f in os.listdir(tmp):
                    if f.endswith(".exr"):
                        size = os.path.getsize(os.path.join(tmp, f))
    lines = [f"drop-in program, {wl['scene']} {wl['width']}x{wl['height']} {wl['samples']} samples, CRAY_HIP_AOV=16 CRAY_HIP_DENOISE=5, frame_ms of CRH_DUMP_STATS (all of renderFrame()), "
             f"three alternating runs behind a warm-up run; the layers file: {size} bytes"]
    for kind, v in times.items():
        lines.append(f"  {kind:40s} median {statistics.median(v):9.2f} ms   ({', '.join(f'{x:.2f}' for x in v)})")
    return lines


def main():
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(REPO, "profiles", "exr_rate.log")
    sys.path.insert(0, REPO)
    from __graft_entry__ import load_package
    gpu = load_package().api.device_count() > 0
    lines = (measure() + ([] if "--no-dropin" in args else dropin())) if gpu else ["no HIP device here: nothing is measured, the register line only"]
    regs = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), "--filter", "k_pack"], capture_output=True, text=True)
    lines += [l for l in regs.stdout.splitlines() if "k_pack" in l] or [f"tools/kernel_regs.py failed: {regs.stderr[-300:]}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
