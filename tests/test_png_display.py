"""The display transform of the GPU PNG — exposure, the four tone curves, the ordered dither (crx_png_pack_display) — and the exposure the device measures from the
frame (crx_auto_exposure), through ZipContext.png / auto_exposure, Context.write_png and the drop-in program's CRAY_HIP_PNG_* variables.

The yardstick is tests/display_spec.py: the header's float32 statements in NumPy, with powf taken from the device's exact_math.h through Context.eval_math, so the
pixels and the exposure must agree bit for bit. The files are read by test_png.py's independent reader (chunk walker, zlib, PIL, the restated filters). CPU tier:
the restatement's own anchors, and this file's GPU tests run by a child pytest on the kernel emulation."""
import ctypes as C
import io
import os
import re
import zlib

import numpy as np
import pytest
from PIL import Image

import display_spec as spec
from support import EMU_DIR, DeviceArray, bits, ctx, dropin_env, dropin_paths, run_gpu_tests_on_emulation  # noqa: F401 (ctx: the fixture)
from test_png import check_png, decode, filtered_data, run_dropin_png, smooth_frame, walk, zctx  # noqa: F401 (zctx: the fixture)

f32 = np.float32
WHITES = [2.0 ** -10, 0.5, 1.0, 4.0, 2.0 ** 10]
POISON = 0xA5


# ---- the CPU tier: the restatement's anchors ------------------------------------------------------------------------------------------------
def test_bayer_matrix_is_a_permutation_with_the_stated_first_row():
    b = spec.bayer_matrix()
    assert b[0].tolist() == [0, 32, 8, 40, 2, 34, 10, 42]
    assert sorted(b.ravel().tolist()) == list(range(64))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cray_hip_exr.h")).read()
    for row in b:          # the 64 numbers stand in the header, row by row
        assert re.search(r"\*\s+" + r"\s+".join(str(v) for v in row) + r"\s*\n", header), row


def test_every_curve_is_finite_and_not_negative_and_white_maps_to_one():
    """Over the whites at the range's ends and inside, x on a log grid up to 2^20 plus the edges, with overflow, invalid operations and divisions by zero raised:
    every y is finite and >= 0; y(white) == 1 for REINHARD and HABLE. (Strict monotonicity does not hold in float32 and is not claimed.)"""
    x = np.concatenate([[0.0, 1e-45, 1e-38, 2.0 ** -40, 1.0, 2.0 ** 20, np.nextafter(f32(2.0 ** 20), f32(0))], np.logspace(-45, np.log10(2.0 ** 20), 20000)]).astype(f32)
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        for white in WHITES:
            for which in range(4):
                y = spec.curve(x, which, white)
                assert y.dtype == f32 and np.isfinite(y).all() and (y >= 0).all(), (which, white)
                big = spec.curve(np.array([3e38, 1e30, 2.0 ** 20 + 1], f32), which, white)
                assert np.isfinite(big).all() and (which == spec.CLAMP or (big == big[0]).all())
            for which in (spec.REINHARD, spec.HABLE):
                assert spec.curve(np.array([white], f32), which, white)[0] == f32(1), (which, white)


def test_key_bin_of_a_sorted_array_holds_the_element_of_that_rank():
    rng = np.random.default_rng(5)
    lum = np.sort(np.exp2(rng.uniform(-20, 12, 5000)).astype(f32))
    fb = np.repeat(lum[:, None], 3, axis=1).reshape(50, 100, 3)          # r = g = b: the luminance is close to the value; the bins are taken from the restatement's own
    binned = np.sort(spec.bins_of(fb))
    assert len(binned) == 5000
    for permille in (1, 250, 500, 999, 1000):
        exposure, key, counted = spec.auto_exposure(fb, permille, 0.18)
        rank = (5000 * permille + 999) // 1000
        assert counted == 5000 and 1 <= rank <= 5000
        k = int(binned[rank - 1])          # the element of rank r, counted from 1
        assert bits(np.array([key]))[0] == (k << 19 | 1 << 18) and exposure == f32(0.18) / key
    assert spec.bins_of(np.full((1, 1, 3), 0.18, f32))[0] in (1990, 1991) and spec.key_of_bin(1991) == f32(0.18359375)
    assert (np.array([0.18], f32).view(np.uint32) >> 19)[0] == 1991
    assert spec.auto_exposure(np.zeros((2, 2, 3), f32), 500, 0.18) == (1, 0, 0)


def test_dither_splits_a_flat_quarter_48_to_16():
    t = np.full((16, 24, 3), 100.25, f32)
    got = spec.bytes_of_t(t, 1)
    for by in range(2):
        for bx in range(3):
            block = got[8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
            assert (block == 100).sum() == 3 * 48 and (block == 99).sum() == 3 * 16
            assert np.array_equal(block[..., 0] == 99, spec.bayer_matrix() < 16)
    assert (spec.bytes_of_t(t, 0) == 100).all()


# ---- the GPU tier ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def powf(ctx):
    return lambda x, y: ctx.eval_math("powf", x, y)


def on_device(pkg, ctx, fb):
    dev = DeviceArray(pkg, fb, np.float32)
    ctx.synchronize()
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (80, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_anchor_and_identity(shape, pkg, ctx, zctx, powf):
    """The restatement under the default display is Context.to_srgb8; png(display=the default) and png(display=None) are png()'s bytes, with both code settings
    and the filters adaptive and paeth."""
    import cray_amd.exrzip as exrzip
    w, h = shape
    fb = smooth_frame(w, h, 3 * w + h)
    dev = on_device(pkg, ctx, fb)
    assert np.array_equal(spec.display_bytes(fb, None, powf), ctx.to_srgb8(dev.ptr, w, h))
    assert np.array_equal(spec.display_bytes(fb, dict(spec.DEFAULT), powf), ctx.to_srgb8(dev.ptr, w, h))
    default = exrzip.Display()
    zctx.L.crx_display_default(C.byref(default))
    assert (default.exposure, default.curve, default.white, default.dither) == (1.0, 0, 4.0, 0)
    try:
        for codes in ("fixed", "dynamic"):
            zctx.set_codes(codes)
            for name in ("adaptive", "paeth"):
                plain = zctx.png(dev.ptr, w, h, name)
                assert zctx.png(dev.ptr, w, h, name, display=None) == plain
                assert zctx.png(dev.ptr, w, h, name, display=default) == plain
                assert zctx.png(dev.ptr, w, h, name, display={}) == plain
                assert zctx.png(dev.ptr, w, h, name, display=dict(white=0.5)) == plain, "white does not enter CLAMP"
    finally:
        zctx.set_codes("fixed")


def planted_frame(w, h, white):
    """smooth_frame with a planted row at the transform's edges"""
    knee, w32, top = f32(0.0031308), f32(white), f32(1048576.0)
    up, down = (lambda v: np.nextafter(f32(v), f32(np.inf))), (lambda v: np.nextafter(f32(v), f32(0)))
    values = np.array([0.0, 1e-45, 1e-38, down(knee), knee, up(knee), 0.18, 1.0, w32, down(w32), up(w32), top, down(top), up(top), 1e30, np.finfo(f32).max], f32)
    fb = smooth_frame(w, h, 5 * w + h)
    assert 3 * w >= values.size and h > 8
    fb.reshape(h, 3 * w)[1, :values.size] = values
    return fb


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(13, 9), (67, 19)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_curve(shape, pkg, ctx, zctx, powf):
    """4 curves x 3 exposures x dither off / on x 2 whites on widths that are multiples of neither 4 nor 8 and more than 8 rows — words straddle pixels, the matrix
    wraps both ways —, with a planted row at every edge of the transform: walk accepts the file, PIL's pixels are the restatement's, the inflated IDAT is the
    restated filtering of those bytes, the frame is not written."""
    w, h = shape
    seen = set()
    for white in (0.5, 4.0):
        fb = planted_frame(w, h, white)
        dev = on_device(pkg, ctx, fb)
        for which in range(4):
            for exposure in (0.25, 1.0, 3.7):
                for dither in (0, 1):
                    d = dict(exposure=exposure, curve=which, white=white, dither=dither)
                    with np.errstate(over="ignore", invalid="ignore"):          # (CLAMP takes FLT_MAX * 3.7 = inf to 255, as linearToSRGB8 does)
                        want8 = spec.display_bytes(fb, d, powf)
                    data = zctx.png(dev.ptr, w, h, "adaptive", display=dict(d, curve=spec.CURVES[which]))
                    got8 = decode(data)
                    if not np.array_equal(got8, want8):
                        bad = np.argwhere(got8 != want8)
                        y, x, c = bad[0]
                        raise AssertionError(f"{d}: {len(bad)} bytes differ, the first at row {y} column {x} component {c}: {got8[y, x, c]}, want {want8[y, x, c]} "
                                             f"for {fb[y, x, c]!r}")
                    check_png(data, w, h, want8, "adaptive")
                    seen.add(want8.tobytes())
        assert np.array_equal(bits(dev.read(ctx)), bits(fb)), "the frame was written"
    assert len(seen) > 40, "the settings hardly change the picture: the inputs degenerated"


def flat_frame(w, h, t_wanted, powf):
    """a constant frame whose t = linearToSRGB(c) * 255 is about t_wanted (the inverse of the sRGB curve, as test_png.linear_of), t checked through the restatement"""
    s = np.float64(t_wanted) / 255.0
    c = f32(s / 12.92 if s <= 0.04045 else ((s + 0.055) / 1.055) ** 2.4)
    fb = np.full((h, w, 3), c, f32)
    t = spec.display_t(fb, None, powf)
    assert np.abs(t - f32(t_wanted)).max() < 0.01, (t_wanted, t[0, 0])
    return fb


@pytest.mark.gpu
def test_dither_placement(pkg, ctx, zctx, powf):
    """A constant 24 x 16 frame at t = k + 0.25: exactly 16 lower pixels per 8 x 8 block, where the matrix is below 16; t = 254.9 stays at 254 / 255, t = 0.1 at 0."""
    w, h = 24, 16
    d = dict(dither=1)
    for k in (100, 7):
        fb = flat_frame(w, h, k + 0.25, powf)
        dev = on_device(pkg, ctx, fb)
        got = decode(zctx.png(dev.ptr, w, h, "none", display=d))
        assert np.array_equal(got, spec.display_bytes(fb, d, powf))
        lower = np.tile(spec.bayer_matrix() < 16, (2, 3))
        for c in range(3):
            assert np.array_equal(got[..., c] == k - 1, lower) and np.array_equal(got[..., c] == k, ~lower)
        for by in range(2):
            for bx in range(3):
                assert (got[8 * by:8 * by + 8, 8 * bx:8 * bx + 8, 0] == k - 1).sum() == 16
    top = flat_frame(w, h, 254.9, powf)
    dev = on_device(pkg, ctx, top)
    got = decode(zctx.png(dev.ptr, w, h, "none", display=d))
    assert np.array_equal(got, spec.display_bytes(top, d, powf)) and set(np.unique(got).tolist()) == {254, 255}
    low = flat_frame(w, h, 0.1, powf)
    dev = on_device(pkg, ctx, low)
    got = decode(zctx.png(dev.ptr, w, h, "none", display=d))
    assert np.array_equal(got, spec.display_bytes(low, d, powf)) and not got.any()


def display_spec_counted(fb):
    return spec.auto_exposure(fb, 500, 0.18)[2]


def same_result(got, want, what):
    assert got[0].dtype == f32 and got[1].dtype == f32
    assert (bits(np.array([got[0]]))[0], bits(np.array([got[1]]))[0], got[2]) == (bits(np.array([want[0]]))[0], bits(np.array([want[1]]))[0], want[2]), (what, got, want)


@pytest.mark.gpu
def test_auto_exposure(pkg, ctx, zctx):
    """crx_auto_exposure, bit for bit the restatement's (exposure, key, counted) for permille 1, 500, 999 and 1000: a constant frame, 1 x 1, 300 x 70 log-uniform
    luminances over 2^-20 .. 2^12 (many workgroups merge), the same with planted NaN, +inf, 0 and negative pixels — counted drops by exactly their number —, pairs
    one ulp apart across a bin boundary, an all-zero frame; two calls agree."""
    rng = np.random.default_rng(12)
    w, h = 300, 70
    wide = (np.exp2(rng.uniform(-20, 12, (h, w, 1))) * rng.uniform(0.5, 1.5, (h, w, 3))).astype(f32)
    planted = wide.copy()
    flat = planted.reshape(-1, 3)
    flat[5] = np.nan; flat[77, 1] = np.nan; flat[1000] = np.inf; flat[1001, 2] = np.inf; flat[2000] = 0.0; flat[2001] = 0.0; flat[3000] = -1.0; flat[20999] = -0.5
    edge = np.array([1990 << 19, 1991 << 19, 2500 << 19, 16 << 19], np.uint32)          # values at bin boundaries and one ulp below, as grey pixels
    pairs = np.concatenate([edge, edge - 1]).view(f32)
    boundary = np.repeat(pairs[:, None], 3, axis=1).reshape(2, 4, 3)
    frames = {"constant": np.full((9, 33, 3), 0.18, f32), "1 x 1": np.array([[[0.5, 0.25, 2.0]]], f32), "log-uniform": wide, "planted": planted,
              "bin boundaries": boundary, "all zero": np.zeros((5, 7, 3), f32), "tiny and huge": np.array([[[1e-45, 0, 0], [3e38, 3e38, 3e38], [1e-30, 1e-30, 1e-30]]], f32)}
    assert len(np.unique(spec.bins_of(wide))) >= 200 and len(np.unique(spec.bins_of(boundary))) >= 4
    assert spec.auto_exposure(planted, 500, 0.18)[2] == w * h - 8 and spec.auto_exposure(wide, 500, 0.18)[2] == w * h
    keys = set()
    for what, fb in frames.items():
        fh, fw, _ = fb.shape
        dev = on_device(pkg, ctx, fb)
        for permille in (1, 500, 999, 1000):
            for target in (0.18, 1.0):
                got = zctx.auto_exposure(dev.ptr, fw, fh, permille, target)
                same_result(got, spec.auto_exposure(fb, permille, target), (what, permille, target))
                same_result(zctx.auto_exposure(dev.ptr, fw, fh, permille, target), got, "a second call")
                keys.add(float(got[1]))
        assert np.array_equal(bits(dev.read(ctx)), bits(fb)), "the frame was written"
    dev = on_device(pkg, ctx, frames["all zero"])
    same_result(zctx.auto_exposure(dev.ptr, 7, 5), (f32(1), f32(0), 0), "all zero")
    assert len(keys) > 12 and zctx.auto_exposure_time_ms() >= 0.0
    # the limits of the exposure
    tiny = on_device(pkg, ctx, np.full((1, 1, 3), 1e-30, f32))
    huge = on_device(pkg, ctx, np.full((1, 1, 3), 1e30, f32))
    assert zctx.auto_exposure(tiny.ptr, 1, 1)[0] == f32(2.0 ** 40) and zctx.auto_exposure(huge.ptr, 1, 1)[0] == f32(2.0 ** -40)


@pytest.mark.gpu
def test_refusals_leave_everything_untouched(pkg, ctx, zctx):
    """CRH_ERR_INVALID for every refusal of the header — crx_png_pack's own, through the new entry, and the display's and the exposure's —; the poisoned output
    buffer, total and result words and the frame stay as they were; the context works afterwards."""
    import cray_amd.exrzip as exrzip
    abi, L = pkg.abi, zctx.L
    w, h = 20, 6
    fb = smooth_frame(w, h, 9)
    dev = on_device(pkg, ctx, fb)
    good = [(b"key", b"value")]
    arr, count = exrzip.png_texts(good)
    bound = C.c_uint64(0)
    assert L.crx_png_bound(w, h, arr, count, C.byref(bound)) == 0
    bound = bound.value
    out = np.full(bound, POISON, np.uint8)
    total = C.c_uint64(0x5A5A5A5A5A5A5A5A)
    nan, inf = float("nan"), float("inf")

    def pack(handle=zctx.h, src=dev.ptr, width=w, height=h, display=(1.5, 2, 4.0, 1), filt=-1, texts=good, count=None, null_list=False, dst=out.ctypes.data,
             capacity=bound, tot=C.byref(total)):
        arr = (exrzip.PngText * max(len(texts), 1))(*[exrzip.PngText(k, v) for k, v in texts])
        d = None if display is None else C.byref(exrzip.Display(*display))
        return L.crx_png_pack_display(handle, src, width, height, d, filt, None if null_list else arr, len(texts) if count is None else count, dst, capacity, tot)
    refused = {
        "NULL context": dict(handle=None), "NULL frame": dict(src=None), "NULL output": dict(dst=None), "NULL total": dict(tot=None),
        "width 0": dict(width=0), "height 0": dict(height=0), "width < 0": dict(width=-w), "height < 0": dict(height=-h),
        "n = 2^31": dict(width=(2 ** 31 // 64 - 1) // 3 + 1, height=64, capacity=2 ** 62), "n far above 2^31": dict(width=2 ** 30, height=2 ** 30, capacity=2 ** 62),
        "filter -2": dict(filt=-2), "filter 5": dict(filt=5),
        "a NULL list with a count": dict(null_list=True, count=1), "an empty key": dict(texts=[(b"", b"v")]), "a key of 80 bytes": dict(texts=[(b"k" * 80, b"v")]),
        "a NULL key": dict(texts=[(None, b"v")]), "a NULL value": dict(texts=good + [(b"k", None)]),
        "capacity below the bound": dict(capacity=bound - 1), "capacity 0": dict(capacity=0),
        "curve -1": dict(display=(1.0, -1, 4.0, 0)), "curve 4": dict(display=(1.0, 4, 4.0, 0)),
        "exposure below 2^-40": dict(display=(float(np.nextafter(f32(2.0 ** -40), f32(0))), 0, 4.0, 0)), "exposure 0": dict(display=(0.0, 2, 4.0, 0)),
        "exposure above 2^40": dict(display=(float(np.nextafter(f32(2.0 ** 40), f32(np.inf))), 0, 4.0, 0)), "exposure < 0": dict(display=(-1.0, 0, 4.0, 0)),
        "exposure NaN": dict(display=(nan, 0, 4.0, 0)), "exposure inf": dict(display=(inf, 0, 4.0, 0)),
        "white below 2^-10": dict(display=(1.0, 1, float(np.nextafter(f32(2.0 ** -10), f32(0))), 0)), "white above 2^10": dict(display=(1.0, 3, 1024.5, 0)),
        "white NaN": dict(display=(1.0, 0, nan, 0)), "white inf": dict(display=(1.0, 1, inf, 0)), "white 0": dict(display=(1.0, 3, 0.0, 0)),
        "dither 2": dict(display=(1.0, 0, 4.0, 2)), "dither -1": dict(display=(1.0, 0, 4.0, -1)),
    }
    for what, kw in refused.items():
        assert pack(**kw) == abi.ERR_INVALID, what
        assert b"crx_png_pack_display" in L.crx_last_error(), what
        assert (out == POISON).all() and total.value == 0x5A5A5A5A5A5A5A5A, what

    result = np.full(4, 0xA5A5A5A5, np.uint32)          # exposure, key, counted (two words)

    def measure(handle=zctx.h, src=dev.ptr, width=w, height=h, permille=500, target=0.18, e=result.ctypes.data, k=result.ctypes.data + 4, n=result.ctypes.data + 8):
        cast = lambda p, t: C.cast(C.c_void_p(p), C.POINTER(t)) if p else None
        return L.crx_auto_exposure(handle, src, width, height, permille, target, cast(e, C.c_float), cast(k, C.c_float), cast(n, C.c_uint64))
    refused = {
        "NULL context": dict(handle=None), "NULL frame": dict(src=None), "NULL exposure": dict(e=None), "NULL key": dict(k=None), "NULL counted": dict(n=None),
        "width 0": dict(width=0), "height < 0": dict(height=-1), "a frame of 2^31 bytes of filtered data": dict(width=2 ** 30, height=2 ** 30),
        "permille 0": dict(permille=0), "permille 1001": dict(permille=1001), "target NaN": dict(target=nan), "target 0": dict(target=0.0), "target < 0": dict(target=-0.18),
        "target inf": dict(target=inf),
    }
    for what, kw in refused.items():
        assert measure(**kw) == abi.ERR_INVALID, what
        assert b"crx_auto_exposure" in L.crx_last_error(), what
        assert (result == 0xA5A5A5A5).all(), what
    ms = C.c_float(7.0)
    assert L.crx_auto_exposure_time_ms(None, C.byref(ms)) == abi.ERR_INVALID and L.crx_auto_exposure_time_ms(zctx.h, None) == abi.ERR_INVALID and ms.value == 7.0
    L.crx_display_default(None)
    assert np.array_equal(bits(dev.read(ctx)), bits(fb)), "the frame was written"
    # the context works afterwards; nothing behind the file or the results is written
    assert pack() == abi.OK and pack(display=None) == abi.OK and measure() == abi.OK
    walk(out[:total.value].tobytes())
    assert total.value <= bound and (out[total.value:] == POISON).all() and result[3] == 0 and result[2] == display_spec_counted(fb)


def display_chunk(data):
    """the payload of the C-ray Display chunk of a file, or None; it is the last tEXt chunk"""
    texts = [p for k, p in walk(data) if k == b"tEXt"]
    found = [p for p in texts if p.startswith(b"C-ray Display\0")]
    assert len(found) <= 1 and (not found or texts[-1] == found[0])
    return found[0].split(b"\0", 1)[1].decode("latin-1") if found else None


@pytest.mark.gpu
def test_write_png_with_a_display_transform(pkg, ctx, zctx, powf, golden_blob, manifest, tmp_path):
    """Context.write_png on the rendered cfg1_scene: with exposure="auto", ACES and the dither the pixels are the restatement's at the exposure auto_exposure returns
    and the C-ray Display chunk parses back to that exposure's bits; with the defaults the file is ZipContext.png's of the call without a display and has no such chunk;
    unknown names raise ValueError."""
    m = manifest["cfg1_scene"]
    w, h = m["width"], m["height"]
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    fb = ctx.framebuffer(w, h)
    ctx.render_region(fb, w, h, 4, 4)
    frame = ctx.download(fb, w, h)
    exposure, key, counted = ctx._zip_context().auto_exposure(fb, w, h, 500, 0.18)
    same_result((exposure, key, counted), spec.auto_exposure(frame, 500, 0.18), "the rendered frame")
    assert counted > w * h // 2 and exposure != 1
    path = str(tmp_path / "display.png")
    text = {"C-ray Samples": "4"}
    size = ctx.write_png(path, w, h, fb, text=text, exposure="auto", tonemap="aces", dither=True)
    data = open(path, "rb").read()
    assert size == len(data)
    want8 = spec.display_bytes(frame, dict(exposure=exposure, curve=spec.ACES, dither=1), powf)
    check_png(data, w, h, want8, "adaptive", texts=[(b"C-ray Samples", b"4"), (b"C-ray Display", display_chunk(data).encode("latin-1"))])
    assert not np.array_equal(want8, ctx.to_srgb8(fb, w, h))
    said = display_chunk(data)
    found = re.fullmatch(r"exposure=(\S+) \(auto 500/1000 of 0\.18\) curve=aces white=4 dither=1", said)
    assert found, said
    assert bits(np.array([f32(found.group(1))]))[0] == bits(np.array([exposure]))[0], (said, exposure)
    assert Image.open(io.BytesIO(data)).info["C-ray Display"] == said
    # a given exposure, another curve, no dither; permille and target reach the measurement
    assert ctx.write_png(path, w, h, fb, exposure=2.5, tonemap="reinhard", white=2.0) > 0
    data = open(path, "rb").read()
    assert display_chunk(data) == "exposure=2.5 curve=reinhard white=2 dither=0"
    assert np.array_equal(decode(data), spec.display_bytes(frame, dict(exposure=2.5, curve=spec.REINHARD, white=2.0), powf))
    ctx.write_png(path, w, h, fb, exposure="auto", auto_permille=900, auto_target=0.5)
    other = ctx._zip_context().auto_exposure(fb, w, h, 900, 0.5)[0]
    assert display_chunk(open(path, "rb").read()) == f"exposure={float(other):.9g} (auto 900/1000 of 0.5) curve=clamp white=4 dither=0" and other != exposure
    # the defaults: the parent's file, no chunk
    default = str(tmp_path / "default.png")
    size = ctx.write_png(default, w, h, fb, text=text)
    z = ctx._zip_context()
    z.set_codes("dynamic")
    try:
        assert open(default, "rb").read() == z.png(fb, w, h, "adaptive", text) and size == os.path.getsize(default)
    finally:
        z.set_codes("fixed")
    assert display_chunk(open(default, "rb").read()) is None
    for kw in (dict(tonemap="filmic"), dict(tonemap=2), dict(exposure="automatic")):
        with pytest.raises(ValueError):
            ctx.write_png(str(tmp_path / "x.png"), w, h, fb, **kw)
    assert not os.path.exists(str(tmp_path / "x.png"))


@pytest.mark.gpu
def test_dropin_program_applies_the_display_transform(pkg, ctx, manifest, golden_blob, tmp_path):
    """c-ray-hip with CRAY_HIP_PNG=1 CRAY_HIP_PNG_EXPOSURE=auto CRAY_HIP_PNG_TONEMAP=hable CRAY_HIP_PNG_DITHER=1: the _gpu_ file's pixels are those of
    Context.write_png with the same arguments on the same scene blob and settings, its third tEXt chunk is the same string, the log names the exposure; with
    CRAY_HIP_PNG_TONEMAP=nonsense a warning, and the file of CRAY_HIP_PNG=1 alone."""
    if not dropin_paths()[2]:
        pytest.skip("c-ray-hip or the asset overlay is not built (needs the reference's sources at build time)")
    m = manifest["cfg1_scene"]
    w, h = m["width"], m["height"]
    env = dict(dropin_env(), CRAY_HIP_PNG="1")
    files, text = run_dropin_png(manifest, str(tmp_path / "display"), dict(env, CRAY_HIP_PNG_EXPOSURE="auto", CRAY_HIP_PNG_TONEMAP="hable", CRAY_HIP_PNG_DITHER="1"))
    data = files["refrun_gpu_0000.png"]
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    fb = ctx.framebuffer(w, h)
    ctx.render_region(fb, w, h, m["samples"], m["bounces"])
    path = str(tmp_path / "api.png")
    ctx.write_png(path, w, h, fb, text=[("C-ray Samples", str(m["samples"])), ("C-ray Bounces", str(m["bounces"]))], exposure="auto", tonemap="hable", dither=True)
    want = open(path, "rb").read()
    assert np.array_equal(decode(data), decode(want))
    texts = [p for k, p in walk(data) if k == b"tEXt"]
    assert len(texts) == 3 and texts == [p for k, p in walk(want) if k == b"tEXt"]
    said = display_chunk(data)
    assert said.startswith("exposure=") and said.endswith(" (auto 500/1000 of 0.18) curve=hable white=4 dither=1") and said in text, (said, text[-1500:])
    assert not np.array_equal(decode(data), decode(files["refrun_0000.png"]))
    plain, _ = run_dropin_png(manifest, str(tmp_path / "plain"), env)
    bad, text = run_dropin_png(manifest, str(tmp_path / "bad"), dict(env, CRAY_HIP_PNG_TONEMAP="nonsense", CRAY_HIP_PNG_DITHER="1"))
    assert bad["refrun_gpu_0000.png"] == plain["refrun_gpu_0000.png"] and "without a display transform" in text
    assert display_chunk(plain["refrun_gpu_0000.png"]) is None


# ---- the CPU tier's run of the above ------------------------------------------------------------------------------------------------------
def test_display_kernels_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the emulation builds of both libraries (powf there is the emulation library's eval_math): every
    one of them runs and passes, none skipped (the drop-in test where the drop-in program is built)."""
    run_gpu_tests_on_emulation(__file__, 10, passed_without_dropin=9, extra_env={"CRX_LIB": os.path.join(EMU_DIR, "libcray_hip_exr_emu.so")},
                               make_targets=("libcray_hip_emu.so", "-f Makefile.exr"), dropin_libs=("libcray_hip_exr.so",))
