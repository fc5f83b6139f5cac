"""The arithmetic of the two denoisers as include/cray_hip.h states it, in NumPy float32 — correctly rounded + - * / sqrt in a fixed order, which the GPU tier holds
the kernels to bit for bit — and the synthetic frames the tests of crh_denoise, crh_denoise_variance and the adaptive sampler filter (a specification and its
inputs: no test lives here; tests/test_denoise.py, tests/test_denoise_variance.py, tests/test_adaptive.py and tests/test_adaptive_cells.py use it)."""
import numpy as np

f32 = np.float32
K = [f32(3 / 8), f32(1 / 4), f32(1 / 16)]
VMAX = f32(2.0 ** 100)


# ---- crh_denoise ----------------------------------------------------------------------------------------------------------------------------
def lum(I):
    return (f32(0.2126) * I[..., 0] + f32(0.7152) * I[..., 1]) + f32(0.0722) * I[..., 2]


def prepare(fb, aov):
    alb, n, d, cov = aov[..., 0:3], aov[..., 3:6], aov[..., 6], aov[..., 7]
    a = np.maximum(alb + (f32(1) - cov)[..., None], f32(2.0 ** -8))
    c = np.where(np.isfinite(fb) & (fb > 0), fb, f32(0))
    I = c / a
    nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
    with np.errstate(all="ignore"):
        nh = np.where((nn > 0)[..., None], n / np.sqrt(nn)[..., None], f32(0))
        z = np.where(cov > 0, d / cov, f32(0))
    Crec = np.concatenate([I, lum(I)[..., None]], -1).astype(f32)
    Grec = np.concatenate([nh, z[..., None]], -1).astype(f32)
    return Crec, Grec, a.astype(f32)


def iteration(Crec, Grec, s, sn, sz, sc):
    H, W, _ = Crec.shape
    acc, ws = np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    one = f32(1)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * s, dx * s
            y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            P, Q = np.s_[y0:y1, x0:x1], np.s_[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
            h = K[abs(dx)] * K[abs(dy)]
            dn = Grec[P][..., 0:3] - Grec[Q][..., 0:3]
            d2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
            t = np.maximum(one - sn * d2, f32(0))
            t2 = t * t
            wn = t2 * t2
            zp, zq = Grec[P][..., 3], Grec[Q][..., 3]
            r = (np.abs(zp - zq) / (np.maximum(zp, zq) + f32(1e-6))) / sz
            wz = one / (one + r * r)
            lp, lq = Crec[P][..., 3], Crec[Q][..., 3]
            e = (lp - lq) / (sc * ((lp + lq) + f32(1e-4)))
            wc = one / (one + e * e)
            w = ((h * wn) * wz) * wc
            acc[P] = acc[P] + w[..., None] * Crec[Q][..., 0:3]
            ws[P] = ws[P] + w
    I = acc / ws[..., None]
    return np.concatenate([I, lum(I)[..., None]], -1).astype(f32)


def restatement(fb, aov, iterations=5, sigma_normal=1.0, sigma_depth=0.05, sigma_color=1.0):
    Crec, Grec, a = prepare(fb, aov)
    for i in range(iterations):
        Crec = iteration(Crec, Grec, 1 << i, f32(sigma_normal), f32(sigma_depth), f32(f32(sigma_color) * f32(2.0 ** -i)))
    out = Crec[..., 0:3] * a
    assert out.dtype == np.float32
    return out


# ---- crh_denoise_variance -----------------------------------------------------------------------------------------------------------------
def windows(H, W, oy, ox):
    """The pixels p whose tap q = p + (ox, oy) is inside the image, and those taps; None when there are none."""
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return np.s_[y0:y1, x0:x1], np.s_[y0 + oy:y1 + oy, x0 + ox:x1 + ox]


def gw(G, P, Q, sn, sz):
    """wn, wz as in iteration()"""
    one = f32(1)
    dn = G[P][..., 0:3] - G[Q][..., 0:3]
    d2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
    t = np.maximum(one - sn * d2, f32(0))
    t2 = t * t
    wn = t2 * t2
    zp, zq = G[P][..., 3], G[Q][..., 3]
    r = (np.abs(zp - zq) / (np.maximum(zp, zq) + f32(1e-6))) / sz
    return wn, one / (one + r * r)


def prefilter(V, G, sn, sz):
    H, W = V.shape
    acc, ws = np.zeros((H, W), f32), np.zeros((H, W), f32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            PQ = windows(H, W, dy, dx)
            if PQ is None:
                continue
            P, Q = PQ
            wn, wz = gw(G, P, Q, sn, sz)
            wg = wn * wz
            acc[P] = acc[P] + wg * V[Q]
            ws[P] = ws[P] + wg
    return acc / ws


def iteration_v(I, V, G, s, sn, sz, sc):
    H, W, _ = I.shape
    one = f32(1)
    L = lum(I)
    den = sc * np.sqrt(V) + f32(1e-4)
    acc, ws, va = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            PQ = windows(H, W, dy * s, dx * s)
            if PQ is None:
                continue
            P, Q = PQ
            h = K[abs(dx)] * K[abs(dy)]
            wn, wz = gw(G, P, Q, sn, sz)
            e = (L[P] - L[Q]) / den[P]
            wc = one / (one + e * e)
            w = ((h * wn) * wz) * wc
            acc[P] = acc[P] + w[..., None] * I[Q]
            ws[P] = ws[P] + w
            va[P] = va[P] + (w * w) * V[Q]
    return acc / ws[..., None], va / (ws * ws)


def restatement_v(fb, half, aov, scale, iterations=5, sigma_normal=1.0, sigma_depth=0.05, sigma_color=3.0):
    Crec, G, a = prepare(fb, aov)
    I = Crec[..., 0:3]
    with np.errstate(all="ignore"):
        Chalf, _, _ = prepare(half, aov)
        d = Chalf[..., 3] - Crec[..., 3]
        v = f32(scale) * (d * d)
    V = np.where(v < VMAX, v, VMAX).astype(f32)          # NaN and inf -> 2^100
    sn, sz, sc = f32(sigma_normal), f32(sigma_depth), f32(sigma_color)
    if iterations:
        V = prefilter(V, G, sn, sz)
    for i in range(iterations):
        I, V = iteration_v(I, V, G, 1 << i, sn, sz, sc)
        assert I.dtype == np.float32 and V.dtype == np.float32
    out = I * a
    assert out.dtype == np.float32
    return out


# ---- the synthetic scene ----------------------------------------------------------------------------------------------------------------
def synthetic(W, H, seed=7):
    """A left wall (normal (1, 0, 0), depth 4 + 0.01 row) and a right plane (normal (0, 0.6, 0.8), depth 7 + 0.02 col) under a top strip of misses; the row
    below the strip is half covered, its albedo, normal and depth pre-multiplied by the coverage as a folded AOV is; a 5-pixel checker albedo; irradiance
    constant per region; multiplicative Gaussian noise of relative sigma 0.2, clamped at 0. Returns noisy, aov, clean, left mask, the half-covered row."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    top = (12 * H) // 70
    left, bg = xx < (45 * W) // 100, yy < top
    aov = np.zeros((H, W, 8), f32)
    nrm = np.where(left[..., None], np.array([1, 0, 0], f32), np.array([0, 0.6, 0.8], f32)).astype(f32)
    depth = np.where(left, f32(4) + f32(0.01) * yy, f32(7) + f32(0.02) * xx).astype(f32)
    alb = ((0.2 + 0.6 * (((xx // 5) + (yy // 5)) % 2))[..., None] * np.array([1, 0.8, 0.6])).astype(f32)
    cov = np.ones((H, W), f32)
    cov[bg] = 0
    cov[top] = 0.5
    aov[..., 0:3], aov[..., 3:6], aov[..., 6], aov[..., 7] = alb * cov[..., None], nrm * cov[..., None], depth * cov, cov
    irr = np.where(left[..., None], np.array([1.5, 1.2, 1.0], f32), np.array([0.3, 0.5, 0.9], f32)).astype(f32)
    clean = (irr * (aov[..., 0:3] + (1 - cov)[..., None])).astype(f32)
    clean[bg] = np.array([0.7, 0.8, 1.0], f32)
    noisy = np.maximum((clean * (1 + 0.2 * rng.standard_normal((H, W, 3)))).astype(f32), f32(0))
    return noisy, aov, clean, left, top


def poisoned(noisy):
    """One NaN, one +inf and one negative channel: the filter's guard maps them to 0."""
    fb = noisy.copy()
    H, W, _ = fb.shape
    fb[H // 2, W // 3, 0] = np.nan
    fb[H // 3, W // 2, 1] = np.inf
    fb[H - 1, W - 1, 2] = -1.0
    return fb


def poisoned_half(noisy):
    """The half-sample frame's own NaN, inf and negative channel, away from the frame's, and one finite value whose irradiance overflows: variance 2^100."""
    half = noisy.copy()
    H, W, _ = half.shape
    half[H // 4, W // 2, 1] = np.nan
    half[(2 * H) // 3, W // 5, 2] = np.inf
    half[0, W - 1, 0] = -2.0
    if W > 1:          # (a single pixel has no channel left)
        half[H - 1, 0, 1] = 3.0e38
    return half
