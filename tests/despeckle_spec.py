"""The firefly filter crx_despeckle as include/cray_hip_exr.h states it, in NumPy float32 — correctly rounded * + / and comparisons in the header's order, which the
GPU tier holds the kernels to bit for bit (a specification: no test lives here; tests/test_despeckle.py uses it). The reference R is taken by sorting, the header's
own statement; clamped_by_count is the kernel's shortcut, restated separately so that a test can hold the two against each other."""
import numpy as np

f32 = np.float32
DEFAULT = dict(radius=2, rank=4, factor=4.0, floor=2.0 ** -6)


def params_of(**params):
    unknown = set(params) - set(DEFAULT)
    if unknown:
        raise TypeError(f"unexpected parameter {sorted(unknown)[0]!r}")
    p = dict(DEFAULT, **params)
    return int(p["radius"]), int(p["rank"]), f32(p["factor"]), f32(p["floor"])


def luminance(fb):
    with np.errstate(all="ignore"):
        return (f32(0.2126) * fb[..., 0] + f32(0.7152) * fb[..., 1]) + f32(0.0722) * fb[..., 2]


def bad_of(fb):
    return ~(np.isfinite(fb).all(axis=-1) & np.isfinite(luminance(fb)))


def guarded(fb):
    L = luminance(fb)
    with np.errstate(invalid="ignore"):
        return np.where(~bad_of(fb) & (L > 0), L, f32(0)).astype(f32)


def neighbours(g, radius):
    """[H, W, (2 radius + 1)^2 - 1] of the neighbours' g, -1 where the neighbour is outside the image, and their number m [H, W]"""
    H, W = g.shape
    padded = np.full((H + 2 * radius, W + 2 * radius), f32(-1), f32)
    padded[radius:radius + H, radius:radius + W] = g
    out = [padded[radius + dy:radius + dy + H, radius + dx:radius + dx + W] for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dx, dy) != (0, 0)]
    nb = np.stack(out, axis=-1)
    return nb, (nb >= 0).sum(axis=-1)


def limit(fb, **params):
    """(T [H, W] — 0 where m == 0 —, m): steps 4 to 7"""
    radius, rank, factor, floor = params_of(**params)
    nb, m = neighbours(guarded(fb), radius)
    k = np.minimum(rank, m)
    descending = -np.sort(-nb, axis=-1)          # the outside's -1 sort last
    R = np.take_along_axis(descending, np.maximum(k - 1, 0)[..., None], axis=-1)[..., 0]
    with np.errstate(over="ignore"):
        T = (factor * R + floor).astype(f32)
    return np.where(m > 0, T, f32(0)).astype(f32), m


def measure(fb, **params):
    """(the plane s [H, W] of float32, clamped, bad): steps 1 to 9"""
    fb = np.asarray(fb)
    assert fb.dtype == f32 and fb.ndim == 3 and fb.shape[2] == 3
    g, bad = guarded(fb), bad_of(fb)
    T, m = limit(fb, **params)
    clamped = ~bad & (m > 0) & (g > T)
    with np.errstate(all="ignore"):
        s = np.where(clamped, T / np.where(clamped, g, f32(1)), f32(1)).astype(f32)
    s[bad] = 0
    assert s.dtype == f32
    return s, clamped, bad


def scale(fb, **params):
    return measure(fb, **params)[0]


def clamped_by_count(fb, **params):
    """which pixels the monotone counting form clamps: not bad, and fewer than k neighbours with (factor * g(q)) + floor >= g(p)"""
    radius, rank, factor, floor = params_of(**params)
    g = guarded(fb)
    nb, m = neighbours(g, radius)
    with np.errstate(over="ignore"):
        reach = ((nb >= 0) & ((factor * nb + floor).astype(f32) >= g[..., None])).sum(axis=-1)
    return ~bad_of(fb) & (reach < np.minimum(rank, m))


def clamped_of(fb, **params):
    return measure(fb, **params)[1]


def apply_scale(frame, s):
    """step 10"""
    with np.errstate(all="ignore"):
        out = (frame * s[..., None]).astype(f32)
    out[s == 0] = 0          # +0.0f
    keep = s == 1
    out[keep] = frame[keep]
    return out


def apply(fb, *also, **params):
    """fb as its own guide: the despeckled fb; with `also`, the tuple of every frame under fb's plane"""
    s = scale(fb, **params)
    frames = tuple(apply_scale(f, s) for f in (fb,) + also)
    return frames if also else frames[0]


def stats(fb, **params):
    (s, clamped, bad), g = measure(fb, **params), guarded(fb)
    return dict(clamped=int(clamped.sum()), bad=int(bad.sum()), max_clamped=f32(g[clamped].max() if clamped.any() else 0),
                min_scale=f32(s[clamped].min() if clamped.any() else 1))
