"""The display transform of the GPU PNG and the automatic exposure, restated in NumPy float32 in the order of operations include/cray_hip_exr.h states (a plain
helper module like denoise_spec.py): display_bytes is what crx_png_pack_display's pixels must be, bit for bit; auto_exposure is crx_auto_exposure. powf comes from
the caller — Context.eval_math("powf", ...), the device's own exact_math.h —, so the sRGB step needs no second statement."""
import numpy as np

f32 = np.float32
CLAMP, REINHARD, ACES, HABLE = 0, 1, 2, 3
CURVES = ("clamp", "reinhard", "aces", "hable")
X_MAX = f32(1048576.0)
EXPOSURE_RANGE = (f32(2.0 ** -40), f32(2.0 ** 40))
WHITE_RANGE = (f32(2.0 ** -10), f32(2.0 ** 10))
DEFAULT = dict(exposure=1.0, curve=CLAMP, white=4.0, dither=0)
BINS = 4096


def bayer(x, y):
    """B(x, y) of the header, built bit by bit: for i = 0, 1, 2, bit 2 (2 - i) + 1 is bit i of x ^ y, bit 2 (2 - i) is bit i of y."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    q, b = x ^ y, np.zeros(np.broadcast(x, y).shape, np.int64)
    for i in range(3):
        b |= ((q >> i) & 1) << (2 * (2 - i) + 1) | ((y >> i) & 1) << (2 * (2 - i))
    return b


def bayer_matrix():
    """[row y, column x]"""
    return bayer(np.arange(8)[None, :], np.arange(8)[:, None])


def hable(v):
    v = np.asarray(v, f32)
    return (v * (f32(0.15) * v + f32(0.05)) + f32(0.004)) / (v * (f32(0.15) * v + f32(0.5)) + f32(0.06)) - f32(0.02) / f32(0.3)


def curve(x, which, white):
    """y of x = exposure * c, float32 [.]"""
    x, white = np.asarray(x, f32), f32(white)
    if which == CLAMP:
        return x
    x = np.where(x < X_MAX, x, X_MAX).astype(f32)
    if which == REINHARD:
        return (x * (f32(1) + x / (white * white))) / (f32(1) + x)
    if which == ACES:
        return (x * (f32(2.51) * x + f32(0.03))) / (x * (f32(2.43) * x + f32(0.59)) + f32(0.14))
    assert which == HABLE
    return hable(f32(2) * x) / hable(f32(2) * white)


def linear_to_srgb(y, powf):
    """srgb8.h's linearToSRGB on float32 y, with the caller's powf(x [n], y [n]) -> [n]"""
    y = np.ascontiguousarray(y, f32)
    flat = y.ravel()
    p = np.asarray(powf(flat, np.full(flat.size, 0.4166666667, f32)), f32).reshape(y.shape)
    return np.where(y <= f32(0.0031308), f32(12.92) * y, (f32(1.055) * p) - f32(0.055)).astype(f32)


def display_t(fb, display, powf):
    """t = linearToSRGB(curve(exposure * c)) * 255, float32, shaped like fb"""
    d = dict(DEFAULT, **(display or {}))
    x = f32(d["exposure"]) * np.asarray(fb, f32)
    return linear_to_srgb(curve(x, d["curve"], d["white"]), powf) * f32(255)


def bytes_of_t(t, dither):
    """the bytes of t [H, W, 3]: the truncating rule, or with the centred ordered offset of the pixel's column and stored row in front of it"""
    t = np.asarray(t, f32)
    if not dither:
        return np.where(t < f32(255), t, f32(255)).astype(f32).astype(np.uint8)
    h, w, _ = t.shape
    yy, xx = np.mgrid[0:h, 0:w]
    off = (bayer(xx & 7, yy & 7).astype(f32) - f32(31.5)) / f32(64)
    u = (t + off[..., None]).astype(f32)
    return np.where(u < 0, 0, np.where(u < f32(255), np.clip(u, 0, 255).astype(np.uint8), 255)).astype(np.uint8)


def display_bytes(fb, display, powf):
    """uint8 [H, W, 3]: the pixels of crx_png_pack_display(fb, display); display: None (the default) or a mapping with any of exposure, curve (0 .. 3), white, dither"""
    d = dict(DEFAULT, **(display or {}))
    return bytes_of_t(display_t(fb, d, powf), d["dither"])


def luminance(fb):
    fb = np.asarray(fb, f32)
    return ((f32(0.2126) * fb[..., 0]) + (f32(0.7152) * fb[..., 1])) + (f32(0.0722) * fb[..., 2])


def bins_of(fb):
    """the bins of the pixels that count (finite luminance > 0): bits >> 19"""
    with np.errstate(over="ignore", invalid="ignore"):
        lum = luminance(fb).ravel().astype(f32)
    lum = lum[np.isfinite(lum) & (lum > 0)]
    return (lum.view(np.uint32) >> 19).astype(np.int64)


def key_of_bin(k):
    return np.array([(int(k) << 19) | (1 << 18)], np.uint32).view(f32)[0]


def auto_exposure(fb, permille, target):
    """(exposure float32, key float32, counted int) of crx_auto_exposure"""
    bins = bins_of(fb)
    n = int(bins.size)
    if n == 0:
        return f32(1), f32(0), 0
    rank = (n * int(permille) + 999) // 1000
    cum = np.cumsum(np.bincount(bins, minlength=BINS))
    k = int(np.searchsorted(cum, rank, side="left"))          # the smallest bin whose cumulative count is >= rank
    key = key_of_bin(k)
    with np.errstate(over="ignore"):
        exposure = f32(target) / key
    return f32(min(max(exposure, EXPOSURE_RANGE[0]), EXPOSURE_RANGE[1])), key, n
