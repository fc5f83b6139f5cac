#!/usr/bin/env python3
"""ids_rate.py — k_ids against k_aov on the same dispatch (scenes/_built/cfg2_hdr.blob, 1280 x 720, 16 passes of 16), and the two consumers at that size:
medians of interleaved launches in one process on one device. Prints the lines profiles/ids_rate.log holds; `--out FILE` also writes them.

    python tools/ids_rate.py [--out profiles/ids_rate.log]
"""
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import load_package, BUILT

pkg = load_package()
api = pkg.api
w, h, n = 1280, 720, 16
ctx = api.Context(0)
ctx.upload(api.Scene(os.path.join(BUILT, "cfg2_hdr.blob")))
aov = ctx.aov_buffer(w, h)
bi, bm = ctx.ids_buffer(w, h), ctx.ids_buffer(w, h)
ranked = torch.zeros((h, w, 6, 2), dtype=torch.float32, device="cuda:0")
matte = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
t = {k: [] for k in ("aov", "ids", "ids_instance_only", "resolve", "matte8", "matte64")}
ROUNDS, WARM = 12, 3
for r in range(WARM + ROUNDS):
    ctx.clear_aov(aov, w, h)
    ctx.render_aov(aov, w, h, n)
    a = ctx.aov_kernel_time_ms()
    ctx.clear_ids(bi, w, h); ctx.clear_ids(bm, w, h)
    ctx.render_ids(bi, bm, w, h, n)
    b = ctx.ids_kernel_time_ms()
    ctx.clear_ids(bi, w, h)
    ctx.render_ids(bi, None, w, h, n)
    c = ctx.ids_kernel_time_ms()
    ctx.resolve_ids(bi, w, h, ranked.data_ptr())
    d = ctx.ids_kernel_time_ms()
    ctx.ids_matte(bi, w, h, list(range(8)), matte.data_ptr())
    e = ctx.ids_kernel_time_ms()
    ctx.ids_matte(bi, w, h, list(range(64)), matte.data_ptr())
    f = ctx.ids_kernel_time_ms()
    if r >= WARM:
        for k, v in zip(t, (a, b, c, d, e, f)):
            t[k].append(v)
ids = ctx.download_ids(bi, w, h)
cov = ctx.download_aov(aov, w, h)[..., 7]
lines = [f"cfg2_hdr.blob {w}x{h}, {n} passes of {n} ({w * h * n} camera rays); {ROUNDS} interleaved rounds behind {WARM} warm-up rounds, one process, one device",
         f"hits: coverage mean {float(cov.mean()):.4f}; id buffer: sum(count) + lost = {int(ids[..., 6:12].sum() + ids[..., 12].sum())}, lost {int(ids[..., 12].sum())}, "
         f"pixels with 1/2/3+ ids {[int(((ids[..., 6:12] != 0).sum(-1) == k).sum()) for k in (1, 2)]} / {int(((ids[..., 6:12] != 0).sum(-1) >= 3).sum())}"]
for k, v in t.items():
    lines.append(f"{k:20s} median {statistics.median(v):8.4f} ms   min {min(v):8.4f}   max {max(v):8.4f}   ({', '.join(f'{x:.3f}' for x in v)})")
ratio = statistics.median(t["ids"]) / statistics.median(t["aov"])
lines.append(f"ratio k_ids (both buffers) / k_aov = {ratio:.3f}   (expectation 1.1: {'met' if ratio <= 1.1 else 'MISSED'})")
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write("\n".join(lines) + "\n")
print("\n".join(lines))
ctx.close()
