"""The firefly filter crx_despeckle — clamp outlier pixels to a rank of their neighbourhood — through ZipContext.despeckle / despeckle_scale, Context.despeckle in
front of the two denoisers, and the drop-in program's CRAY_HIP_DESPECKLE.

The yardstick is tests/despeckle_spec.py: the header's float32 statements in NumPy, the reference taken by sorting, so the plane, the frames and the stats must agree
bit for bit. CPU tier: the restatement's own anchors, the motivating case on denoise_spec's synthetic scene, and this file's GPU tests run by a child pytest on the
kernel emulation."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_spec
import despeckle_spec as spec
from support import EMU_DIR, DeviceArray, bits, ctx, dropin_env, dropin_paths, run_dropin, run_gpu_tests_on_emulation, same_bits  # noqa: F401 (ctx: the fixture)
from test_png import smooth_frame, zctx  # noqa: F401 (zctx: the fixture)

f32 = np.float32
POISON = 0xA5A5A5A5
SHAPES = [(1, 1), (2, 3), (5, 5), (33, 9), (80, 17)]          # (33, 9): one 32 x 8 tile seam in x and one in y; (80, 17): two in each
# (radius, rank, factor, floor)
SETS = [(2, 4, 4.0, 2.0 ** -6), (1, 1, 1.0, 0.0), (1, 8, 2.0, 0.0), (2, 24, 1.5, 2.0 ** -6), (2, 1, 1.0, 2.0 ** -6), (2, 8, 16.0, 2.0 ** -6)]
SEEDS = {(33, 9): 3, (80, 17): 3}          # chosen so that the condition in test_plane_frames_and_stats holds; it is asserted there from the restatement


def params(s):
    return dict(radius=s[0], rank=s[1], factor=s[2], floor=s[3])


def random_frame(w, h, seed=None):
    """exp(normal(0, 1.5)) per component: luminances over some four decades, a firefly in every neighbourhood for the stricter sets"""
    rng = np.random.default_rng(SEEDS.get((w, h), 1) if seed is None else seed)
    return np.exp(rng.normal(0.0, 1.5, (h, w, 3))).astype(f32)


def tied_frame(w, h):
    """grey pixels at multiples of 1 / 2, so that nearly every window holds its reference several times, with a NaN pixel and an infinite component"""
    grey = np.round(random_frame(w, h, seed=5)[..., 0] * 2) / 2
    fb = np.repeat(grey[..., None], 3, axis=2).astype(f32)
    fb[3, 3], fb[0, w - 1, 1] = np.nan, np.inf
    return fb


def ulps(a, b):
    return abs(int(bits(np.array([a], f32))[0]) - int(bits(np.array([b], f32))[0]))


# ---- the CPU tier: the restatement's anchors ------------------------------------------------------------------------------------------------
def test_a_planted_pixel_on_a_flat_field_comes_down_to_the_limit():
    """9 x 7 of (0.5, 0.25, 0.125) with one pixel 1000 times as bright: its new luminance is the limit factor * flat + floor to within two ulps, the scale has
    the bits T / g(p) gives, the colour ratios stay, every other word is untouched."""
    colour = np.array([0.5, 0.25, 0.125], f32)
    fb = np.tile(colour, (7, 9, 1)).astype(f32)
    fb[3, 4] = colour * f32(1000)
    flat, g = spec.luminance(fb)[0, 0], spec.luminance(fb)[3, 4]
    T = f32(f32(4) * flat + f32(2.0 ** -6))
    s = spec.scale(fb)
    assert bits(s[3, 4:5])[0] == bits(np.array([T / g], f32))[0] and 0 < s[3, 4] < 1
    assert (np.delete(s.ravel(), 3 * 9 + 4) == 1).all()
    out = spec.apply(fb)
    assert ulps(spec.luminance(out)[3, 4], T) <= 2
    assert np.array_equal(bits(out[3, 4]), bits(fb[3, 4] * s[3, 4]))
    assert out[3, 4, 0] / out[3, 4, 1] == 2 and out[3, 4, 1] / out[3, 4, 2] == 2          # (powers of two: the ratios are exact)
    untouched = np.ones((7, 9), bool)
    untouched[3, 4] = False
    assert np.array_equal(bits(out[untouched]), bits(fb[untouched]))
    assert spec.stats(fb) == dict(clamped=1, bad=0, max_clamped=g, min_scale=s[3, 4])


def test_effective_rank():
    """2 x 3 under radius 2 and rank 8: every pixel has 5 neighbours and the reference is the smallest of them; a 1 x 1 image is never clamped."""
    grey = np.array([[1, 2], [4, 8], [16, 32]], f32)
    fb = np.repeat(grey[..., None], 3, axis=2)
    g = spec.guarded(fb)
    T, m = spec.limit(fb, radius=2, rank=8, factor=1.0, floor=0.0)
    assert (m == 5).all()
    for y in range(3):
        for x in range(2):
            assert T[y, x] == np.delete(g.ravel(), 2 * y + x).min()
    assert np.array_equal(spec.clamped_of(fb, radius=2, rank=8, factor=1.0, floor=0.0), g > g.min())
    for value in (1e30, np.inf, np.nan, 0.0):
        one = np.full((1, 1, 3), value, f32)
        assert not spec.clamped_of(one).any() and spec.scale(one)[0, 0] == (1 if np.isfinite(value) else 0)


def test_ties_need_no_rule():
    """a pixel whose neighbours are all equal has that value as its reference, whatever the rank"""
    fb = np.full((5, 5, 3), 0.25, f32)
    fb[2, 2] = 100.0
    g = spec.guarded(fb)
    for rank in (1, 4, 24):
        T, _ = spec.limit(fb, rank=rank, factor=1.0, floor=0.0)
        assert T[2, 2] == g[0, 0]
    T, _ = spec.limit(fb, rank=1, factor=1.0, floor=0.0)
    assert T[1, 1] == g[2, 2] and spec.limit(fb, rank=2, factor=1.0, floor=0.0)[0][1, 1] == g[0, 0]


def test_the_counting_form_equals_the_selection_form():
    """the kernel's shortcut — fewer than k neighbours whose limit reaches g(p) — clamps exactly the pixels the sorted reference clamps, on the GPU tier's frames and
    sets and on a frame with ties and bad pixels"""
    for fb in [random_frame(w, h) for w, h in SHAPES] + [tied_frame(40, 12)]:
        for s in SETS:
            assert np.array_equal(spec.clamped_by_count(fb, **params(s)), spec.clamped_of(fb, **params(s))), (fb.shape, s)


def test_smooth_frames_are_left_alone():
    for w, h in [(1, 1), (2, 3), (80, 17), (37, 29)]:
        fb = smooth_frame(w, h, 3 * w + h)
        got = spec.stats(fb)
        assert got["clamped"] == 0 and got["bad"] == 0, (w, h, got)
        assert np.array_equal(bits(spec.apply(fb)), bits(fb))


def planted_synthetic():
    noisy, aov, clean, _, _ = denoise_spec.synthetic(64, 40)
    planted = noisy.copy()
    where = [(20, 10), (30, 40), (3, 50)]          # the wall, the plane, the strip of misses
    for y, x in where:
        planted[y, x] = noisy[y, x] * f32(200) + f32(50)
    return noisy, planted, aov, clean, where


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)))


def test_the_denoiser_keeps_fireflies_and_the_filter_removes_them():
    """The motivating case on denoise_spec.synthetic(64, 40) with three pixels planted at fb * 200 + 50: all three are clamped at the defaults and nothing of the
    unplanted frame is; the denoised frame's RMSE against `clean` falls by at least a factor of 10 when the filter runs first (here 0.78 without, 0.0062 with —
    against 0.0062 for the frame without plants)."""
    noisy, planted, aov, clean, where = planted_synthetic()
    assert spec.stats(noisy)["clamped"] == 0
    c = spec.clamped_of(planted)
    assert c.sum() == 3 and all(c[y, x] for y, x in where)
    kept, removed = rmse(denoise_spec.restatement(planted, aov), clean), rmse(denoise_spec.restatement(spec.apply(planted), aov), clean)
    print(f"RMSE of the denoised frame against clean: {kept:.4f} with the fireflies, {removed:.4f} despeckled first")
    assert removed * 10 <= kept


def test_unknown_parameter_names_raise():
    with pytest.raises(TypeError):
        spec.scale(np.zeros((1, 1, 3), f32), sigma=1.0)


# ---- the GPU tier ---------------------------------------------------------------------------------------------------------------------------
def on_device(pkg, ctx, fb):
    dev = DeviceArray(pkg, fb, np.float32)
    ctx.synchronize()
    return dev


def same_stats(got, want, what):
    assert set(got) == set(want) and got["max_clamped"].dtype == f32 and got["min_scale"].dtype == f32
    key = lambda d: (d["clamped"], d["bad"], int(bits(np.array([d["max_clamped"]], f32))[0]), int(bits(np.array([d["min_scale"]], f32))[0]))
    assert key(got) == key(want), (what, got, want)


def check_against_the_restatement(pkg, ctx, zctx, fb, what, **p):
    """despeckle(guide = the frame itself) on a device copy: the plane, the frame and the stats are the restatement's; returns the plane"""
    h, w, _ = fb.shape
    with np.errstate(all="ignore"):
        want_s, want_fb, want_stats = spec.scale(fb, **p), spec.apply(fb, **p), spec.stats(fb, **p)
    dev = on_device(pkg, ctx, fb)
    got_stats = zctx.despeckle(dev.ptr, w, h, (dev.ptr,), **p)
    same_bits(zctx.despeckle_scale(w, h), want_s, f"{what}: the plane")
    same_bits(dev.read(ctx), want_fb, f"{what}: the frame")
    same_stats(got_stats, want_stats, what)
    return want_s


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plane_frames_and_stats(shape, pkg, ctx, zctx):
    """exp(normal(0, 1.5)) frames under the six parameter sets: bit for bit the restatement's plane, frame and stats. From 33 x 9 on every set clamps at least 3
    pixels and leaves at least a tenth unclamped (asserted from the restatement before anything is compared)."""
    w, h = shape
    fb = random_frame(w, h)
    for s in SETS:
        share = spec.clamped_of(fb, **params(s))
        if w * h >= 33 * 9:
            assert share.sum() >= 3 and (~share).mean() >= 0.1, (shape, s, int(share.sum()), share.size)
        check_against_the_restatement(pkg, ctx, zctx, fb, f"{w}x{h} {s}", **params(s))


@pytest.mark.gpu
def test_ties(pkg, ctx, zctx):
    """40 x 12 of luminances quantised to a handful of values, so that nearly every window holds its reference several times, with a NaN and an infinity planted:
    the selection on the device counts with multiplicity as the sorted reference does."""
    w, h = 40, 12
    fb = tied_frame(w, h)
    assert len(np.unique(spec.guarded(fb))) < w * h // 8
    for s in SETS:
        assert spec.clamped_of(fb, **params(s)).sum() >= 3, s
        check_against_the_restatement(pkg, ctx, zctx, fb, f"ties {s}", **params(s))


def edge_pixels():
    sub = np.array([1, 2, 3], np.uint32).view(f32)          # subnormals
    return {"a NaN component": [0.5, np.nan, 0.5], "+inf": [np.inf, 1.0, 1.0], "-inf": [1.0, 1.0, -np.inf], "a negative component, positive luminance": [50.0, -1.0, 50.0],
            "all negative": [-1.0, -2.0, -3.0], "all zero": [0.0, 0.0, 0.0], "a subnormal": list(sub)}


BAD_KINDS = ("a NaN component", "+inf", "-inf")


@pytest.mark.gpu
def test_edge_pixels(pkg, ctx, zctx):
    """80 x 17 with a NaN component, +inf, -inf, a negative component under a positive luminance, an all-negative pixel, an all-zero pixel, and a subnormal, each in turn at the four corners, at x = 31 / 32 and at y = 7 / 8 (the tile seams): the restatement's bits; a bad pixel comes
    out as three +0.0f words and the stats count them."""
    w, h = 80, 17
    kinds = edge_pixels()
    places = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (3, 31), (3, 32), (7, 50), (8, 50)]
    names = list(kinds)
    for turn in range(len(names)):
        fb = random_frame(w, h, seed=20 + turn)
        for i, (y, x) in enumerate(places):
            fb[y, x] = np.array(kinds[names[(i + turn) % len(names)]], f32)
        bad = spec.bad_of(fb)
        count = sum(names[(i + turn) % len(names)] in BAD_KINDS for i in range(len(places)))          # 3, or 4 where the turn repeats one of them
        assert bad.sum() == count and spec.stats(fb)["bad"] == count and count >= 3
        for s in (SETS[0], SETS[1]):
            plane = check_against_the_restatement(pkg, ctx, zctx, fb, f"turn {turn} {s}", **params(s))
            assert (plane[bad] == 0).all()
        dev = on_device(pkg, ctx, fb)
        assert zctx.despeckle(dev.ptr, w, h, (dev.ptr,))["bad"] == count
        assert (bits(dev.read(ctx))[bad] == 0).all(), "a bad pixel is three +0.0f words"


@pytest.mark.gpu
def test_in_place_and_shared(pkg, ctx, zctx):
    """frames = (guide, other): both are scaled by the guide's plane, a third buffer that was not passed stays bit-identical, and where the plane reads 1 both
    frames keep their bits — negative zeros and NaNs of `other` included."""
    w, h = 80, 17
    fb, other = random_frame(w, h), random_frame(w, h, seed=9)
    p = params(SETS[0])
    s = spec.scale(fb, **p)
    kept, scaled = np.argwhere(s == 1), np.argwhere(s != 1)
    assert len(kept) >= 2 and len(scaled) >= 3
    other[tuple(kept[0])], other[tuple(kept[-1])], other[tuple(scaled[0])] = np.nan, -0.0, np.inf
    want_fb, want_other = spec.apply(fb, other, **p)
    dfb, dother, dthird = on_device(pkg, ctx, fb), on_device(pkg, ctx, other), on_device(pkg, ctx, other)
    zctx.despeckle(dfb.ptr, w, h, (dfb.ptr, dother.ptr), **p)
    got_fb, got_other = dfb.read(ctx), dother.read(ctx)
    same_bits(got_fb, want_fb, "the guide")
    same_bits(got_other, want_other, "the other frame")
    same_bits(dthird.read(ctx), other, "a buffer that was not passed")
    assert np.array_equal(bits(got_fb)[s == 1], bits(fb)[s == 1]) and np.array_equal(bits(got_other)[s == 1], bits(other)[s == 1])
    measure_ms, apply_ms = zctx.despeckle_time_ms()
    assert measure_ms >= 0.0 and apply_ms >= 0.0


@pytest.mark.gpu
def test_measure_only(pkg, ctx, zctx):
    """frame_count 0 leaves the guide untouched; despeckle_scale then returns the plane, and refuses another size"""
    w, h = 33, 9
    fb = random_frame(w, h)
    dev = on_device(pkg, ctx, fb)
    same_stats(zctx.despeckle(dev.ptr, w, h), spec.stats(fb), "measure only")
    same_bits(dev.read(ctx), fb, "the guide")
    same_bits(zctx.despeckle_scale(w, h), spec.scale(fb), "the plane")
    with pytest.raises(ValueError):
        zctx.despeckle_scale(h, w)
    with pytest.raises(TypeError):
        zctx.despeckle(dev.ptr, w, h, sigma=1.0)


@pytest.mark.gpu
def test_determinism(pkg, ctx, zctx):
    """two calls on fresh copies give equal planes, frames and stats (a call on another shape in between)"""
    w, h = 80, 17
    fb = random_frame(w, h)
    seen = []
    for _ in range(2):
        dev = on_device(pkg, ctx, fb)
        stats = zctx.despeckle(dev.ptr, w, h, (dev.ptr,), **params(SETS[2]))
        seen.append((zctx.despeckle_scale(w, h), dev.read(ctx), stats))
        small = on_device(pkg, ctx, random_frame(5, 5))
        zctx.despeckle(small.ptr, 5, 5, (small.ptr,))
    same_bits(seen[1][0], seen[0][0], "the plane")
    same_bits(seen[1][1], seen[0][1], "the frame")
    same_stats(seen[1][2], seen[0][2], "the stats")
    assert seen[0][2]["clamped"] > 100


@pytest.mark.gpu
def test_refusals_leave_everything_untouched(pkg, ctx, zctx):
    """CRH_ERR_INVALID for every refusal of the header; the poisoned frames, the stats words and the scale's output stay as they were; the context works afterwards."""
    import cray_amd.exrzip as exrzip
    abi, L = pkg.abi, zctx.L
    w, h = 20, 6
    poison = np.full((h, w, 3), POISON, np.uint32).view(f32)
    guide, a, b = on_device(pkg, ctx, poison), on_device(pkg, ctx, poison), on_device(pkg, ctx, poison)
    stats = np.full(6, POISON, np.uint32)          # two uint64 and two floats
    nan, inf = float("nan"), float("inf")
    default = exrzip.DespeckleParams()
    L.crx_despeckle_default(C.byref(default))
    L.crx_despeckle_default(None)
    assert (default.radius, default.rank, default.factor, default.floor) == (2, 4, 4.0, 2.0 ** -6)

    def call(handle=zctx.h, p=(2, 4, 4.0, 2.0 ** -6), src=guide.ptr, width=w, height=h, frames=(a.ptr, b.ptr), count=None, null_list=False, out=stats.ctypes.data):
        arr = (C.c_void_p * max(len(frames), 1))(*frames)
        q = None if p is None else C.byref(exrzip.DespeckleParams(*p))
        return L.crx_despeckle(handle, q, src, width, height, None if null_list else arr, len(frames) if count is None else count,
                               C.cast(C.c_void_p(out), C.POINTER(exrzip.DespeckleStats)) if out else None)
    refused = {
        "NULL context": dict(handle=None), "NULL guide": dict(src=None), "width 0": dict(width=0), "height 0": dict(height=0), "width < 0": dict(width=-w),
        "height < 0": dict(height=-h), "a frame of 2^31 bytes of filtered data": dict(width=(2 ** 31 // 64 - 1) // 3 + 1, height=64),
        "a frame far above that": dict(width=2 ** 30, height=2 ** 30),
        "radius 0": dict(p=(0, 1, 4.0, 0.0)), "radius 3": dict(p=(3, 4, 4.0, 0.0)), "rank 0": dict(p=(2, 0, 4.0, 0.0)), "rank 25": dict(p=(2, 25, 4.0, 0.0)),
        "rank 9 at radius 1": dict(p=(1, 9, 4.0, 0.0)), "rank < 0": dict(p=(2, -1, 4.0, 0.0)),
        "factor below 1": dict(p=(2, 4, float(np.nextafter(f32(1), f32(0))), 0.0)), "factor above 2^20": dict(p=(2, 4, float(np.nextafter(f32(2.0 ** 20), f32(np.inf))), 0.0)),
        "factor NaN": dict(p=(2, 4, nan, 0.0)), "factor inf": dict(p=(2, 4, inf, 0.0)), "factor < 0": dict(p=(2, 4, -4.0, 0.0)),
        "floor < 0": dict(p=(2, 4, 4.0, -1e-30)), "floor above 2^20": dict(p=(2, 4, 4.0, 2.0 ** 20 + 1)), "floor NaN": dict(p=(2, 4, 4.0, nan)), "floor inf": dict(p=(2, 4, 4.0, inf)),
        "9 frames": dict(frames=(a.ptr,) * 9), "a NULL list with a count": dict(null_list=True, count=1), "a NULL entry": dict(frames=(a.ptr, None)),
    }
    for what, kw in refused.items():
        assert call(**kw) == abi.ERR_INVALID, what
        assert b"crx_despeckle" in L.crx_last_error(), what
        assert (stats == POISON).all(), what
    for dev in (guide, a, b):
        assert (bits(dev.read(ctx)) == POISON).all(), "a refused call wrote a frame"
    plane = np.full(w * h, POISON, np.uint32)
    fresh = exrzip.ZipContext(0)
    try:
        assert L.crx_despeckle_scale(fresh.h, plane.ctypes.data) == abi.ERR_INVALID and b"crx_despeckle_scale" in L.crx_last_error()
        assert call(handle=fresh.h, width=0) == abi.ERR_INVALID and L.crx_despeckle_scale(fresh.h, plane.ctypes.data) == abi.ERR_INVALID
        ms = (C.c_float * 2)(7.0, 7.0)
        assert L.crx_despeckle_time_ms(fresh.h, ms) == abi.OK and list(ms) == [0.0, 0.0]
    finally:
        fresh.close()
    assert L.crx_despeckle_scale(None, plane.ctypes.data) == abi.ERR_INVALID and L.crx_despeckle_scale(zctx.h, None) == abi.ERR_INVALID
    assert L.crx_despeckle_time_ms(None, (C.c_float * 2)()) == abi.ERR_INVALID and L.crx_despeckle_time_ms(zctx.h, None) == abi.ERR_INVALID
    assert (plane == POISON).all()
    # the context works afterwards: the range's ends are taken, NULL params are the defaults, NULL stats are allowed
    fb = random_frame(w, h)
    for p in ((1, 8, 1.0, 0.0), (2, 24, 2.0 ** 20, 2.0 ** 20)):
        dev = on_device(pkg, ctx, fb)
        assert call(p=p, src=dev.ptr, frames=(dev.ptr,)) == abi.OK
        same_bits(dev.read(ctx), spec.apply(fb, **params(p)), f"{p}")
    dev = on_device(pkg, ctx, fb)
    assert call(p=None, src=dev.ptr, frames=(dev.ptr,), out=None) == abi.OK
    same_bits(dev.read(ctx), spec.apply(fb), "NULL params")
    assert L.crx_despeckle_scale(zctx.h, plane.ctypes.data) == abi.OK
    same_bits(plane.view(f32).reshape(h, w), spec.scale(fb), "the plane through the C entry")


@pytest.mark.gpu
def test_context_despeckle_in_front_of_the_denoisers(pkg, ctx):
    """Context.despeckle then Context.denoise on the planted synthetic scene is restatement(spec.apply(...)) bit for bit; Context.despeckle(also=(half,)) then
    denoise_variance is restatement_v of the two frames under the one plane. The returned stats are the restatement's."""
    noisy, planted, aov, clean, where = planted_synthetic()
    planted[10, 20, 1] = np.nan
    h, w, _ = planted.shape
    dfb, daov, dout = on_device(pkg, ctx, planted), on_device(pkg, ctx, aov), on_device(pkg, ctx, np.zeros_like(planted))
    same_stats(ctx.despeckle(dfb.ptr, w, h), spec.stats(planted), "Context.despeckle")
    same_bits(dfb.read(ctx), spec.apply(planted), "the despeckled frame")
    ctx.denoise(dfb.ptr, daov.ptr, w, h, out=dout.ptr)
    same_bits(dout.read(ctx), denoise_spec.restatement(spec.apply(planted), aov), "despeckle, then denoise")
    half = denoise_spec.synthetic(64, 40, seed=11)[0]
    half[where[0]] = planted[where[0]] * f32(1.5)
    want_fb, want_half = spec.apply(planted, half, rank=2)
    dfb, dhalf = on_device(pkg, ctx, planted), on_device(pkg, ctx, half)
    assert ctx.despeckle(dfb.ptr, w, h, also=(dhalf.ptr,), rank=2)["clamped"] == spec.stats(planted, rank=2)["clamped"]
    same_bits(dhalf.read(ctx), want_half, "the half-sample frame under the frame's plane")
    ctx.denoise_variance(dfb.ptr, dhalf.ptr, daov.ptr, w, h, 4, 8, out=dout.ptr)
    same_bits(dout.read(ctx), denoise_spec.restatement_v(want_fb, want_half, aov, f32(4) / f32(4)), "despeckle, then denoise_variance")
    with pytest.raises(TypeError):
        ctx.despeckle(dfb.ptr, w, h, sigma=1.0)


@pytest.mark.gpu
def test_dropin_program_despeckles_the_denoisers_input(pkg, ctx, manifest, golden_blob, tmp_path):
    """c-ray-hip with CRAY_HIP_DENOISE=3 CRAY_HIP_DESPECKLE=4 on cfg1_scene: the denoised dump equals Context.despeckle + Context.denoise on the dumped frame, the
    frame's own dump is that of the run without the variable, the two denoised dumps differ (the 4-pass frame has about 1 % of clamped pixels), one log line gives
    the counts; a bad value: a warning and the plain denoise; without CRAY_HIP_DENOISE: a warning and the same frame."""
    if not dropin_paths()[2]:
        pytest.skip("c-ray-hip or the asset overlay is not built (needs the reference's sources at build time)")
    m = manifest["cfg1_scene"]
    w, h, s = m["width"], m["height"], m["samples"]
    env = dict(dropin_env(), CRH_DUMP_F32=str(tmp_path / "frame.f32"), CRH_DUMP_DENOISED_F32=str(tmp_path / "denoised.f32"), CRAY_HIP_DENOISE="3")
    plain, _ = run_dropin(manifest, tmp_path, env)
    files, text = run_dropin(manifest, tmp_path, dict(env, CRAY_HIP_DESPECKLE="4"))
    assert files["frame.f32"] == plain["frame.f32"], "the frame itself is untouched"
    assert sorted(files) == sorted(plain)
    assert all(files[f] == plain[f] for f in files if f.endswith(".bmp") and "_denoised" not in f), "the frame's image changed"
    frame = np.frombuffer(files["frame.f32"], f32).reshape(h, w, 3)
    got = np.frombuffer(files["denoised.f32"], f32).reshape(h, w, 3)
    want_stats = spec.stats(frame)
    assert want_stats["clamped"] > w * h // 1000
    assert f"{want_stats['clamped']} pixels clamped, {want_stats['bad']} bad" in text, text[-1500:]
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    buf = ctx.aov_buffer(w, h)
    ctx.render_aov(buf, w, h, s, pass_count=min(16, s))
    dfb, dout = on_device(pkg, ctx, frame), on_device(pkg, ctx, np.zeros_like(frame))
    same_stats(ctx.despeckle(dfb.ptr, w, h), want_stats, "the dumped frame")
    ctx.denoise(dfb.ptr, buf, w, h, out=dout.ptr, iterations=3)
    same_bits(got, dout.read(ctx), "drop-in")
    assert (bits(got) != bits(np.frombuffer(plain["denoised.f32"], f32).reshape(h, w, 3))).any()
    bad, text = run_dropin(manifest, tmp_path, dict(env, CRAY_HIP_DESPECKLE="0.5"))
    assert bad["denoised.f32"] == plain["denoised.f32"] and "the frame is denoised as it is" in text
    env.pop("CRAY_HIP_DENOISE")
    os.remove(tmp_path / "denoised.f32")
    alone, text = run_dropin(manifest, tmp_path, dict(env, CRAY_HIP_DESPECKLE="4"))
    assert alone["frame.f32"] == plain["frame.f32"] and "denoised.f32" not in alone and "has no effect without CRAY_HIP_DENOISE" in text


# ---- the CPU tier's run of the above ------------------------------------------------------------------------------------------------------
def test_despeckle_kernels_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the emulation builds of both libraries: every one of them runs and passes, none skipped (the
    drop-in test where the drop-in program is built)."""
    run_gpu_tests_on_emulation(__file__, 13, passed_without_dropin=12, extra_env={"CRX_LIB": os.path.join(EMU_DIR, "libcray_hip_exr_emu.so")},
                               make_targets=("libcray_hip_emu.so", "-f Makefile.exr"), dropin_libs=("libcray_hip_exr.so",))
