#!/usr/bin/env python3
"""exr_zip_rate.py — what the ZIP / ZIPS compressed layers file costs and saves on the frame of tools/exr_rate.py: the bench scene (the cfg2 blob bench.py uses) at
1280 x 720 with all 38 channels — the frame, the guides, a denoised frame and both ranked ID buffers.

    python tools/exr_zip_rate.py [--out profiles/exr_zip_rate.log]
    python tools/exr_zip_rate.py --half [--out profiles/exr_half_rate.log]
    python tools/exr_zip_rate.py --half --codes dynamic [--out ...]

One process, behind warm-up rounds, medians of interleaved rounds of
  zip, zips     crx_pack_zip over the whole frame in one call (lines_per_chunk 16 and 1): the kernels per phase by crx_pack_zip_phases_ms (the companion library's
                events around its four launches), the wall time of the whole call (map upload, kernels, sizes, copy through pinned memory, copy out), and the
                wall time of exr.file_bytes + the file's write to a temporary directory;
  none          the wall time of Context.pack_scanlines on the same buffers and of exr.file_bytes + the file's write.
Then, once, the yardstick: host zlib, level 1, fixed codes (Z_FIXED), per chunk on the same transformed bytes, raw where not shorter, on one thread.
Two expectations are marked met or refuted: the compressed call + write is no slower end to end than the uncompressed one, and the device's size is within a few
percent (5 %) of the yardstick's. Without a GPU nothing is measured and the log says so.

--half adds, interleaved with those in the same rounds, the rows of the file whose colour layers are HALF (Context.write_layers_exr(half=True)'s set, 12 of the 38
channels): "zip half", "zips half" and "none half" through crx_pack (compression 3, 2 and 0) with the same phases, call and write times and file bytes, the spread
between the rounds of every kernel sum, and two more expectations: the half call's kernel time is no larger than the all-FLOAT call's by more than that spread,
and the half file is smaller for every compression (the ratio is recorded).

--codes dynamic adds, interleaved in the same rounds again, the rows of crx_set_codes(CRX_CODES_DYNAMIC): "zip dynamic" and "zips dynamic" (with --half also "zip half
dynamic" and "zips half dynamic") — phases, call and write times, the file's bytes as a share of raw and of the fixed-codes file, the deflate kernel's time beside the
fixed kernel's of the same rounds — and a second host yardstick: zlib level 1 with the default strategy (dynamic codes allowed) per chunk on the same T'. The
expectation "no slower end to end than the uncompressed output" is marked for the dynamic rows too."""
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PASSES, BOUNCES, GUIDE_PASSES, ROUNDS, WARM = 1280, 720, 16, 8, 16, 7, 2
PHASES = ("gather + transform", "deflate", "sizes and offsets", "compaction")


def zip_forward(raw):
    r = np.frombuffer(raw, np.uint8)
    t = np.concatenate([r[0::2], r[1::2]])
    p = t.copy()
    p[1:] = t[1:] - t[:-1] + np.uint8(128)
    return p.tobytes()


def measure(half=False, dynamic=False):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from __graft_entry__ import load_package
    from denoise_rate import blob_path
    pkg = load_package()
    api, exr = pkg.api, pkg.exr
    import cray_amd.exrzip as exrzip
    ctx = api.Context(0)
    scene = api.Scene(blob_path())
    ctx.upload(scene)
    fb, dn, aov = ctx.framebuffer(W, H), ctx.framebuffer(W, H), ctx.aov_buffer(W, H)
    bi, bm, ri, rm = (ctx.ids_buffer(W, H) for _ in range(4))
    ctx.render_region(fb, W, H, PASSES, BOUNCES)
    ctx.render_aov(aov, W, H, PASSES, pass_count=GUIDE_PASSES)
    ctx.render_ids(bi, bm, W, H, PASSES, pass_count=GUIDE_PASSES)
    ctx.denoise(fb, aov, W, H, out=dn)
    ctx.resolve_ids(bi, W, H, ri)
    ctx.resolve_ids(bm, W, H, rm)
    inst = [f"instance#{i}" for i in range(int(scene.desc.instance_count))]
    mat = [f"material#{i}" for i in range(int(scene.desc.material_count))]
    chans = exr.layer_channels(fb, aov, dn, ri, rm, exr.id_map(inst), exr.id_map(mat))
    names = [c[0] for c in chans]
    strings = dict(exr.crypto_attributes("CryptoObject", inst), **exr.crypto_attributes("CryptoMaterial", mat))
    n = len(chans)
    ctx.synchronize()
    zctx = exrzip.ZipContext(0)
    kinds = ("zip", "zips", "none") + (("zip half", "zips half", "none half") if half else ())
    if dynamic:
        kinds += ("zip dynamic", "zips dynamic") + (("zip half dynamic", "zips half dynamic") if half else ())
    types = exr.half_types(names, True)
    t = {k: {"call": [], "write": [], "phases": []} for k in kinds}
    size, device = {}, {}          # the files' bytes; the bytes of the device's chunks
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(WARM + ROUNDS):
            for kind in kinds:
                t0 = time.perf_counter()
                if kind == "none":
                    blocks = ctx.pack_scanlines([c[1:] for c in chans], W, H)
                elif kind != "zip" and kind != "zips":
                    zctx.set_codes("dynamic" if kind.endswith("dynamic") else "fixed")
                    data, sizes = zctx.pack([c[1:] for c in chans], W, H, exrzip.COMPRESSION[kind.split()[0]][0], types if "half" in kind else None)
                    zctx.set_codes("fixed")
                else:
                    data, sizes = zctx.pack_zip([c[1:] for c in chans], W, H, exrzip.COMPRESSION[kind][1])
                t1 = time.perf_counter()
                if kind == "none":
                    whole = exr.file_bytes(W, H, names, blocks, strings=strings)
                else:
                    whole = exr.file_bytes(W, H, names, data, sizes, strings, exrzip.COMPRESSION[kind.split()[0]][0], types if "half" in kind else None)
                with open(os.path.join(tmp, "layers.exr"), "wb") as f:
                    f.write(whole)
                t2 = time.perf_counter()
                size[kind] = len(whole)
                if kind != "none":
                    device[kind] = len(data)
                if r >= WARM:
                    t[kind]["call"].append((t1 - t0) * 1e3)
                    t[kind]["write"].append((t2 - t1) * 1e3)
                    if kind != "none":
                        t[kind]["phases"].append(zctx.phases_ms())
    raw = np.frombuffer(blocks, np.uint8).reshape(H, 8 + 4 * n * W)[:, 8:].tobytes()
    lines = [f"{os.path.basename(blob_path())} {W}x{H}, {n} channels, {len(raw)} raw bytes; segment {exrzip.segment_bytes()} bytes; {ROUNDS} interleaved rounds behind {WARM} warm-up "
             f"rounds, one process, one device"]
    med = statistics.median
    for kind in ("zip", "zips"):
        ph = np.median(np.array(t[kind]["phases"]), axis=0)
        lines.append(f"{kind:5s} kernels (crx_pack_zip_phases_ms): " + ", ".join(f"{name} {v:.3f} ms" for name, v in zip(PHASES, ph)) + f"; sum {ph.sum():.3f} ms")
    for kind in ("zip", "zips", "none"):
        c, w = med(t[kind]["call"]), med(t[kind]["write"])
        lines.append(f"{kind:5s} whole call (wall) median {c:9.3f} ms (min {min(t[kind]['call']):.3f}, max {max(t[kind]['call']):.3f});  file bytes + write median {w:9.3f} ms;  "
                     f"together {c + w:9.3f} ms;  file {size[kind]} bytes = {size[kind] / size['none']:.4f} of the uncompressed file")
    yard = {}
    for kind in ("zip", "zips"):
        per = 4 * n * W * exrzip.COMPRESSION[kind][1]
        t0 = time.perf_counter()
        got = 0
        for at in range(0, len(raw), per):
            chunk = raw[at:at + per]
            c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
            got += 8 + min(len(c.compress(zip_forward(chunk)) + c.flush()), len(chunk))
        yard[kind] = got
        lines.append(f"{kind:5s} yardstick (host zlib level 1, Z_FIXED, one thread, transform included): {got} bytes of chunks in {(time.perf_counter() - t0) * 1e3:.0f} ms; "
                     f"the device's chunks: {device[kind]} bytes = {device[kind] / got:.4f} of the yardstick's")
    none_ms = med(t["none"]["call"]) + med(t["none"]["write"])
    for kind in ("zip", "zips"):
        ms = med(t[kind]["call"]) + med(t[kind]["write"])
        lines.append(f"expectation: the compressed output ({kind}) is no slower end to end than the uncompressed one: {ms:.1f} ms against {none_ms:.1f} ms: {'met' if ms <= none_ms else 'REFUTED'}")
    for kind in ("zip", "zips"):
        chunks = device[kind]
        lines.append(f"expectation: the device's size ({kind}) is within 5 % of the yardstick's: {chunks / yard[kind]:.4f} at segment {exrzip.segment_bytes()}: "
                     f"{'met' if chunks <= 1.05 * yard[kind] else 'REFUTED'}")
    if half:
        lines += half_lines(t, size)
    if dynamic:
        lines += dynamic_lines(t, size, device, raw, n, types if half else None, exr, exrzip, none_ms)
    zctx.close()
    ctx.close()
    return lines


def half_lines(t, size):
    """the rows of --half: the files whose colour layers are HALF beside the all-FLOAT ones of the same rounds"""
    med = statistics.median
    lines = [f"half: R G B, albedo.R/G/B, normal.X/Y/Z, denoised.R/G/B stored as HALF (12 of the channels), through crx_pack; the rows above are the all-FLOAT files of the same rounds"]
    sums = {}
    for kind in ("zip", "zips", "none"):
        k = kind + " half"
        ph = np.median(np.array(t[k]["phases"]), axis=0)
        sums[k] = np.array(t[k]["phases"]).sum(axis=1)
        lines.append(f"{k:10s} kernels (crx_pack_zip_phases_ms): " + ", ".join(f"{name} {v:.3f} ms" for name, v in zip(PHASES, ph)) + f"; sum {ph.sum():.3f} ms")
    for kind in ("zip", "zips"):
        sums[kind] = np.array(t[kind]["phases"]).sum(axis=1)
    for k in ("zip", "zips", "zip half", "zips half", "none half"):
        lines.append(f"{k:10s} kernel sum per round: median {med(sums[k]):.3f} ms, min {sums[k].min():.3f}, max {sums[k].max():.3f} (spread {sums[k].max() - sums[k].min():.3f} ms)")
    for kind in ("zip", "zips", "none"):
        k = kind + " half"
        c, w = med(t[k]["call"]), med(t[k]["write"])
        lines.append(f"{k:10s} whole call (wall) median {c:9.3f} ms (min {min(t[k]['call']):.3f}, max {max(t[k]['call']):.3f});  file bytes + write median {w:9.3f} ms;  "
                     f"together {c + w:9.3f} ms;  file {size[k]} bytes = {size[k] / size[kind]:.4f} of the all-FLOAT {kind} file")
    for kind in ("zip", "zips"):
        k = kind + " half"
        spread = max(sums[kind].max() - sums[kind].min(), sums[k].max() - sums[k].min())
        a, b = med(sums[k]), med(sums[kind])
        lines.append(f"expectation (a): the half call's kernel time ({kind}) is no larger than the all-FLOAT call's by more than the spread between the rounds: "
                     f"{a:.3f} ms against {b:.3f} ms, spread {spread:.3f} ms: {'met' if a <= b + spread else 'REFUTED'}")
    for kind in ("zip", "zips", "none"):
        k = kind + " half"
        lines.append(f"expectation (b): the half file ({kind}) is smaller than the all-FLOAT one: {size[k]} against {size[kind]} bytes, ratio {size[k] / size[kind]:.4f}: "
                     f"{'met' if size[k] < size[kind] else 'REFUTED'}")
    return lines


def dynamic_lines(t, size, device, raw, n, types, exr, exrzip, none_ms):
    """the rows of --codes dynamic beside the fixed-codes rows of the same rounds; types: the HALF set where --half is given"""
    med = statistics.median
    lines = ["codes: crx_set_codes(CRX_CODES_DYNAMIC) — per 4 096-byte segment the cheaper of the fixed codes and a dynamic code built on the device; the parse is run twice"]
    rows = [("zip", None), ("zips", None)] + ([("zip half", types), ("zips half", types)] if types is not None else [])
    planes = np.frombuffer(raw, "<u4").reshape(H, n, W)
    for kind, tt in rows:
        k = kind + " dynamic"
        ph, ph0 = np.median(np.array(t[k]["phases"]), axis=0), np.median(np.array(t[kind]["phases"]), axis=0)
        d = np.array(t[k]["phases"])[:, 1]
        lines.append(f"{k:18s} kernels (crx_pack_zip_phases_ms): " + ", ".join(f"{name} {v:.3f} ms" for name, v in zip(PHASES, ph)) + f"; sum {ph.sum():.3f} ms; "
                     f"deflate {ph[1]:.3f} ms (min {d.min():.3f}, max {d.max():.3f}) against {ph0[1]:.3f} ms with fixed codes = {ph[1] / ph0[1]:.2f} x")
    for kind, tt in rows:
        k = kind + " dynamic"
        c, w = med(t[k]["call"]), med(t[k]["write"])
        none = "none half" if tt is not None else "none"
        lines.append(f"{k:18s} whole call (wall) median {c:9.3f} ms (min {min(t[k]['call']):.3f}, max {max(t[k]['call']):.3f});  file bytes + write median {w:9.3f} ms;  "
                     f"together {c + w:9.3f} ms;  file {size[k]} bytes = {size[k] / size[none]:.4f} of the uncompressed file, {size[k] / size[kind]:.4f} of the fixed-codes file")
    for kind, tt in rows:
        lpc = exrzip.COMPRESSION[kind.split()[0]][1]
        if tt is None:
            typed = planes.reshape(H, -1).view(np.uint8)
        else:
            typed = np.concatenate([(exr.half_bits(planes[:, c]).astype("<u2") if v else planes[:, c]).view(np.uint8).reshape(H, -1) for c, v in enumerate(tt)], axis=1)
        t0 = time.perf_counter()
        got = {zlib.Z_FIXED: 0, zlib.Z_DEFAULT_STRATEGY: 0}
        for y in range(0, H, lpc):
            chunk = typed[y:y + lpc].tobytes()
            tp = zip_forward(chunk)
            for strategy in got:
                c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, strategy)
                got[strategy] += 8 + min(len(c.compress(tp) + c.flush()), len(chunk))
        yf, yd = got[zlib.Z_FIXED], got[zlib.Z_DEFAULT_STRATEGY]
        lines.append(f"{kind:10s} yardsticks (host zlib level 1 per chunk on the same T', one thread, {(time.perf_counter() - t0) * 1e3:.0f} ms for both): Z_FIXED {yf} bytes, default strategy "
                     f"(dynamic codes allowed) {yd} bytes = {yd / yf:.4f} of it; the device's chunks: fixed {device[kind]} = {device[kind] / yf:.4f} of Z_FIXED's, "
                     f"dynamic {device[kind + ' dynamic']} = {device[kind + ' dynamic'] / yd:.4f} of the default strategy's and {device[kind + ' dynamic'] / device[kind]:.4f} of its own fixed")
    for kind, tt in rows:
        k = kind + " dynamic"
        ms = med(t[k]["call"]) + med(t[k]["write"])
        lines.append(f"expectation: the compressed output ({k}) is no slower end to end than the uncompressed one: {ms:.1f} ms against {none_ms:.1f} ms: {'met' if ms <= none_ms else 'REFUTED'}")
    return lines


def main():
    args = sys.argv[1:]
    half = "--half" in args
    dynamic = "--codes" in args and args[args.index("--codes") + 1] == "dynamic"
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(REPO, "profiles", "exr_half_rate.log" if half else "exr_zip_rate.log")
    sys.path.insert(0, REPO)
    from __graft_entry__ import load_package
    gpu = load_package().api.device_count() > 0
    lines = measure(half, dynamic) if gpu else ["no HIP device here: nothing is measured"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
