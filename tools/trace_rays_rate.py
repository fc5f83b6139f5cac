#!/usr/bin/env python3
"""trace_rays_rate.py — what a crh_trace_rays call costs (k_trace_rays between its two copies): scenes/_built/cfg3_venus.blob, 2^21 rays from the camera position
spread around the viewing direction (the spread of the tests' camera_rays), medians of the host clock around the call in one process on one device. The entry has
no events of its own, so the figure is the call's — allocation, both copies and the kernel; under `rocprofv3 --kernel-trace --stats -- python tools/trace_rays_rate.py`
the profiler's table gives the kernel alone. Prints its lines; `--out FILE` also writes them. CRH_LIB=<library> measures another build.

    python tools/trace_rays_rate.py [--out FILE]
"""
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
from __graft_entry__ import load_package, BUILT
import oracle_py

N, ROUNDS, WARM, SEED = 1 << 21, 12, 3, 7
api = load_package().api
blob = os.path.join(BUILT, "cfg3_venus.blob")
ctx = api.Context(0)
ctx.upload(api.Scene(blob))
oscene = oracle_py.OracleScene(blob)
rng = np.random.default_rng(SEED)
A = np.array(list(oscene.desc.camera.A), dtype=np.float64).reshape(3, 4)
local = np.stack([rng.normal(size=N) * 0.35, rng.normal(size=N) * 0.25, np.ones(N)], axis=1)
rays = np.zeros((N, 6), np.float32)
rays[:, 0:3] = A[:, 3]
rays[:, 3:6] = (local @ A[:, :3].T).astype(np.float32)
ms = []
for r in range(WARM + ROUNDS):
    t0 = time.perf_counter()
    hits = ctx.trace_rays(rays)
    if r >= WARM:
        ms.append((time.perf_counter() - t0) * 1e3)
lines = [f"cfg3_venus.blob, {N} rays from the camera; {ROUNDS} calls behind {WARM} warm-up calls, one process, one device; hits {int((hits['inst'] >= 0).sum())}, "
         f"node tests {int(hits['node_tests'].sum())}, triangle tests {int(hits['tri_tests'].sum())}",
         f"trace_rays_call      median {statistics.median(ms):8.4f} ms   min {min(ms):8.4f}   max {max(ms):8.4f}   ({', '.join(f'{x:.3f}' for x in ms)})"]
print("\n".join(lines))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write("\n".join(lines) + "\n")
ctx.close()
