"""The arithmetic of crh_adaptive_step as include/cray_hip.h states it, in NumPy float32 — the same enumeration of a tile's pixels, the same 256 strided partial
sums, the same tree, which the GPU tier holds k_adaptive_step to bit for bit — and the inputs, tile lists and drop-in runs that the rectangle-granular and the
cell-granular tests share (a specification and its inputs: no test lives here; tests/test_adaptive.py and tests/test_adaptive_cells.py use it)."""
import os

import numpy as np

import support
from denoise_spec import poisoned, poisoned_half, synthetic

f32 = np.float32
EMAX = f32(2.0 ** 100)
INF = float("inf")
W2, H2, CAP = 160, 100, 16          # the rendered scene of both files: glowmetal at 160 x 100, at most 16 passes
TILE = (64, 40)          # cfg1_scene at 320 x 200: 5 x 5 tiles


# ---- the restatement (include/cray_hip.h: crh_adaptive_step) ---------------------------------------------------------------------------------
def guard(a):
    return np.where(np.isfinite(a) & (a > 0), a, f32(0)).astype(f32)


def pixel_errors(fb, half):
    """e of every pixel, [H, W] in stored order."""
    F, A = guard(fb), guard(half)
    with np.errstate(all="ignore"):
        d = (np.abs(F[..., 0] - A[..., 0]) + np.abs(F[..., 1] - A[..., 1])) + np.abs(F[..., 2] - A[..., 2])
        s = (F[..., 0] + F[..., 1]) + F[..., 2]
        e = d / np.sqrt(s + f32(1e-4))
        e = np.where(e < EMAX, e, EMAX).astype(f32)
    assert e.dtype == np.float32
    return e


def tile_error(e, H, tile):
    """E of one tile: thread t adds e_k for k = t, t + 256, ... in ascending order, then the tree over the 256 partials."""
    x0, y0, x1, y1 = tile
    ek = e[H - y1:H - y0, x0:x1].ravel()          # stored rows H - y1 .. H - 1 - y0 ascending, x ascending within a row
    n = ek.size
    P = np.zeros(256, f32)
    for first in range(0, n, 256):
        m = min(256, n - first)
        P[:m] = P[:m] + ek[first:first + m]
    stride = 128
    while stride >= 1:
        P[:stride] = P[:stride] + P[stride:2 * stride]
        stride //= 2
    E = P[0] / f32(n)
    assert E.dtype == np.float32
    return E


def restatement(fb, half, tiles, threshold):
    """errors float32 [n], flags bool [n], and the half-sample frame afterwards."""
    H = fb.shape[0]
    e = pixel_errors(fb, half)
    errors = np.array([tile_error(e, H, t) for t in tiles], f32)
    flags = ~(errors <= f32(threshold))
    after = half.copy()
    for (x0, y0, x1, y1), go in zip(tiles, flags):
        if go:
            after[H - y1:H - y0, x0:x1] = fb[H - y1:H - y0, x0:x1]
    return errors, flags, after


# ---- tiles and frames -------------------------------------------------------------------------------------------------------------------
def grid(pkg, w, h, tw, th):
    return pkg.tiles.quantize_image(w, h, tw, th, pkg.tiles.ORDER_NORMAL)


def tile_lists(pkg):
    whole = lambda w, h: [(0, 0, w, h)]
    cut = grid(pkg, 161, 75, 64, 64)                                 # 3 x 2 tiles, ragged on the right (33 wide) and at the top (11 high: y counts from the bottom)
    sparse = [t for i, t in enumerate(cut) if i not in (1, 3)] + [(70, 5, 99, 31)]          # two tiles left out, a rectangle inside one of the holes
    corners = [(0, 0, 1, 1), (160, 0, 161, 1), (0, 74, 1, 75), (160, 74, 161, 75)]
    return {"1x1": (1, 1, whole(1, 1)), "3x2": (3, 2, whole(3, 2)), "37x29": (37, 29, whole(37, 29)), "300x5": (300, 5, whole(300, 5)),
            "161x75-64x64": (161, 75, cut), "161x75-sparse": (161, 75, sparse), "161x75-corners": (161, 75, corners)}


_frames = {}


def frames(w, h):
    """The poisoned synthetic frame of a shape and a poisoned second realisation of it as the half-sample frame (made once, never modified)."""
    if (w, h) not in _frames:
        fb, half = poisoned(synthetic(w, h)[0]), poisoned_half(synthetic(w, h, seed=11)[0])
        if w > 2 and h > 2:          # a pixel whose sum overflows: d and sqrt(s) are both inf, e is a NaN and takes the clamp's second branch
            fb[1, 1, 0:2] = 3.0e38
        for a in (fb, half):
            a.setflags(write=False)
        _frames[(w, h)] = (fb, half)
    return _frames[(w, h)]


def two_noise_levels(w, h, n, seed=7):
    """n samples of the synthetic scene with a relative sigma of 0.6 on the left half of the image and 0.05 on the right: the mean of all of them and of the first n / 2."""
    clean = synthetic(w, h)[2]
    rs = np.where(np.mgrid[0:h, 0:w][1] < w // 2, 0.6, 0.05)[..., None]
    rng = np.random.default_rng(seed)
    samples = [np.maximum(clean * (1 + rs * rng.standard_normal(clean.shape)), 0) for _ in range(n)]
    return np.mean(samples, 0).astype(f32), np.mean(samples[:n // 2], 0).astype(f32)


# ---- the drop-in program ------------------------------------------------------------------------------------------------------------------------
def run_dropin(manifest, out_dir, extra_env):
    """c-ray-hip on cfg1_scene with 64 x 40 tiles and `extra_env`, its images in out_dir: the frame's floats, the image files written, the output."""
    m = manifest["cfg1_scene"]
    files, text = support.run_dropin(manifest, out_dir, dict(extra_env, CRH_DUMP_F32=os.path.join(out_dir, "frame.f32")), tile=TILE)
    frame = np.frombuffer(files["frame.f32"], np.float32).reshape(m["height"], m["width"], 3)
    return frame, {f: data for f, data in files.items() if f.endswith(".bmp")}, text


def api_threshold_and_frame(pkg, ctx, manifest, golden_blob, tiles):
    """cfg1_scene through the API over `tiles`, min_passes 2 of its 4 samples: the median error of a measure-only step at 2 passes, and render_adaptive's frame
    and pass counts at that threshold."""
    m = manifest["cfg1_scene"]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    assert s == 4
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    fb, half = ctx.framebuffer(w, h), ctx.framebuffer(w, h)
    ctx.render_tiles(fb, w, h, s, b, tiles, first_pass=0, pass_count=1)
    ctx.copy_framebuffer(fb, half, w, h)
    ctx.render_tiles(fb, w, h, s, b, tiles, first_pass=1, pass_count=1)
    first, _ = ctx.adaptive_step(fb, half, w, h, tiles, INF)
    threshold = float(np.median(first))
    ctx.clear(fb, w, h)
    ctx.clear(half, w, h)
    passes, _ = ctx.render_adaptive(fb, half, w, h, s, b, tiles, min_passes=2, threshold=threshold)
    assert (passes == 2).any() and (passes == 4).any()
    return threshold, ctx.download(fb, w, h), passes


def strip_cut_rectangles(w, h, devices):
    """What the program's GPU threads decide on when there are several: GPU g's 4-row strips (every devices-th one), cut every tileWidth columns."""
    return [(x, y, min(x + TILE[0], w), min(y + 4, h)) for g in range(devices) for i, y in enumerate(range(0, h, 4)) if i % devices == g for x in range(0, w, TILE[0])]
