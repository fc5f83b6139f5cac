"""The guided à-trous denoiser (crh_denoise, c-ray_amd/csrc/denoise.h): the frame, demodulated by the first-hit albedo, filtered with the 5 x 5 B3-spline taps
at steps 1, 2, 4, ... under normal, depth and luminance weights.

The filter's arithmetic is part of the interface (include/cray_hip.h): correctly rounded float32 + - * / sqrt in a fixed order. tests/denoise_spec.py's
`restatement` is that arithmetic in NumPy float32, and the GPU tier holds the kernels to it bit for bit — on a synthetic scene at shapes that leave every tiling path (single pixel,
smaller than the footprint, ragged tiles, steps larger than the image) and on a rendered frame with its own guides. Two properties are checked without the
restatement: nothing leaks across a normal edge, and the noise goes down by the factor a five-level wavelet filter must reach. The CPU tier runs this file's GPU
tests on the kernel emulation (tests/emu: the same kernel source on a HIP shim)."""
import ctypes as C
import os

import numpy as np
import pytest

from denoise_spec import poisoned, restatement, synthetic
from support import DeviceArray, assert_bit_equal, bits, ctx, dropin_env, dropin_paths, f32, header_values, run_dropin, run_gpu_tests_on_emulation  # noqa: F401 (ctx: the fixture)

DEFAULTS = dict(iterations=5, sigma_normal=1.0, sigma_depth=0.05, sigma_color=1.0)


_cache = {}


def case(W, H, **params):
    """The poisoned synthetic frame of a shape, its guides and the restatement's answer (computed once per shape and parameter set, never modified)."""
    key = (W, H, tuple(sorted(params.items())))
    if key not in _cache:
        noisy, aov, _, _, _ = synthetic(W, H)
        fb = poisoned(noisy)
        want = restatement(fb, aov, **params)
        for a in (fb, aov, want):
            a.setflags(write=False)
        _cache[key] = (fb, aov, want)
    return _cache[key]


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------
def gpu_denoise(pkg, ctx, fb, aov, in_place=False, **params):
    """Context.denoise on copies of fb and aov: the output; out of place, the inputs must come back untouched."""
    h, w = fb.shape[:2]
    dfb, daov = DeviceArray(pkg, fb), DeviceArray(pkg, aov)
    if in_place:
        ctx.denoise(dfb.ptr, daov.ptr, w, h, **params)
        out = dfb.read(ctx)
    else:
        dout = DeviceArray(pkg, np.full((h, w, 3), -7.0, np.float32))
        ctx.denoise(dfb.ptr, daov.ptr, w, h, out=dout.ptr, **params)
        out = dout.read(ctx)
        assert np.array_equal(bits(dfb.read(ctx)), bits(fb)), "the frame was written"
    assert np.array_equal(bits(daov.read(ctx)), bits(aov)), "the guides were written"
    return out


# ---- 1. bit equality with the restatement ----------------------------------------------------------------------------------------------------
# 161 x 75: more than two 32 x 8 tiles plus halo in both directions, no multiple of any tile up to 64 x 32; 37 x 29: at steps 8 and 16 most taps are outside
SHAPE_CASES = [
    pytest.param(1, 1, dict(iterations=5), False, id="1x1"),
    pytest.param(3, 2, dict(iterations=5), False, id="3x2"),
    pytest.param(37, 29, dict(iterations=5), True, id="37x29-in-place"),
    pytest.param(161, 75, dict(iterations=5), False, id="161x75"),
    pytest.param(100, 70, dict(iterations=0), False, id="100x70-0"),
    pytest.param(100, 70, dict(iterations=1), False, id="100x70-1"),
    pytest.param(100, 70, dict(iterations=3, sigma_normal=0.7, sigma_depth=0.11, sigma_color=2.5), False, id="100x70-3-sigmas"),
    pytest.param(100, 70, dict(iterations=8), False, id="100x70-8"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,params,in_place", SHAPE_CASES)
def test_output_equals_the_restatement_bit_for_bit(w, h, params, in_place, pkg, ctx):
    fb, aov, want = case(w, h, **params)
    assert not np.isfinite(fb).all() and (fb < 0).any(), "the frame holds a NaN, an inf and a negative channel"
    got = gpu_denoise(pkg, ctx, fb, aov, in_place=in_place, **params)
    assert_bit_equal(got, want, f"{w}x{h} {params}")


@pytest.mark.gpu
@pytest.mark.parametrize("forms", ["dddddddd", "ttttdddd", "llllllll"], ids=["direct", "dense-tiles", "sub-lattice"])
def test_every_form_of_the_iteration_kernel_equals_the_restatement(forms, pkg, ctx):
    """The library picks a form of the iteration kernel per step (denoise.h: direct gather, dense LDS tile, sub-lattice LDS tile); CRH_DENOISE_FORM forces
    one letter per iteration. Every form at every step it exists for, on the ragged shape, 8 iterations (steps 1 .. 128: beyond the image at the end). The
    product library holds the direct form and the LDS tile whose records are one apart (the dense tile of step 1 = the sub-lattice tile of every step); the dense
    tiles of the steps 2, 4, 8 exist in the emulation tier's build and in A/B builds, elsewhere their letter leaves the step to the default form."""
    w, h, params = 161, 75, dict(iterations=8)
    fb, aov, want = case(w, h, **params)
    os.environ["CRH_DENOISE_FORM"] = forms
    try:
        got = gpu_denoise(pkg, ctx, fb, aov, **params)
    finally:
        del os.environ["CRH_DENOISE_FORM"]
    assert_bit_equal(got, want, f"forms {forms}")


# ---- 2. on a rendered frame ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rendered_frame_equals_the_restatement(pkg, ctx, manifest, golden_blob):
    """glowmetal at 160 x 100, 4 passes of 4 and 4 passes of guides, the defaults: context-owned buffers, in place."""
    w, h, n = 160, 100, 4
    ctx.upload(pkg.api.Scene(golden_blob("glowmetal")))
    fb, buf = ctx.framebuffer(w, h), ctx.aov_buffer(w, h)
    ctx.render_region(fb, w, h, n, manifest["glowmetal"]["bounces"])
    ctx.render_aov(buf, w, h, n)
    frame, aov = ctx.download(fb, w, h), ctx.download_aov(buf, w, h)
    cov = aov[..., 7]
    partial = int(((cov > 0) & (cov < 1)).sum())
    print(f"{partial} partially covered pixels")
    assert partial > 0 and frame.any()
    ctx.denoise(fb, buf, w, h)
    got = ctx.download(fb, w, h)
    assert_bit_equal(got, restatement(frame, aov), "glowmetal")
    assert (bits(got) != bits(frame)).any()


# ---- 3. edges hold (independent of the restatement) ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nothing_leaks_across_a_normal_edge(pkg, ctx):
    """The right plane three times as bright: the left wall's output below the half-covered row does not change by one bit — the normal weight across that edge
    is exactly 0 (|n - n'|^2 = 2 between wall and plane, 1 against a miss: t = max(1 - 1 * d2, 0) = 0)."""
    w, h = 100, 70
    noisy, aov, _, left, top = synthetic(w, h)
    yy = np.mgrid[0:h, 0:w][0]
    first = gpu_denoise(pkg, ctx, noisy, aov)
    brighter = noisy.copy()
    brighter[~left] *= f32(3)
    second = gpu_denoise(pkg, ctx, brighter, aov)
    sel = left & (yy > top)
    assert sel.sum() > 2000
    assert np.array_equal(bits(first[sel]), bits(second[sel])), f"{(bits(first[sel]) != bits(second[sel])).sum()} floats of the wall changed"
    assert (bits(first[~left]) != bits(second[~left])).any(), "the plane itself did change"


# ---- 4. it denoises ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_noise_goes_down_tenfold(pkg, ctx):
    """RMSE(out, clean) / RMSE(noisy, clean) <= 0.10 with the defaults. The restatement gives 0.037 at 5 iterations, 0.080 at 3 and 0.286 at 1 (one B3 pass on
    iid noise: 0.273 in theory), so a filter that stops early or never widens its step fails; the margin is for the seed, not for the device."""
    w, h = 100, 70
    noisy, aov, clean, _, _ = synthetic(w, h)
    out = gpu_denoise(pkg, ctx, noisy, aov)

    def rmse(a):
        return float(np.sqrt(((a.astype(np.float64) - clean.astype(np.float64)) ** 2).mean()))
    ratio = rmse(out) / rmse(noisy)
    print(f"rmse noisy {rmse(noisy):.5f} denoised {rmse(out):.5f} ratio {ratio:.4f}")
    assert ratio <= 0.10, ratio


# ---- 5. entry points ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_entry_point_behaviour(pkg, manifest, golden_blob, tmp_path):
    api, abi = pkg.api, pkg.abi
    L = api.library()
    if api.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device; libcray_hip has no CPU fallback")
    assert abi.ABI_VERSION == 5 and L.crh_abi_version() == 5
    # the struct as the header lays it out, and its defaults
    size, version = header_values(tmp_path, "sizeof(crh_denoise_params)", "CRH_ABI_VERSION")
    assert size == C.sizeof(abi.DenoiseParams) == 24 and version == 5
    p = abi.DenoiseParams(-1, -1, -1, -1.0, -1.0, -1.0)
    L.crh_denoise_params_default(C.byref(p))
    assert (p.iterations, p.sigma_normal, p.sigma_depth, p.sigma_color) == (5, 1.0, f32(0.05), 1.0)
    L.crh_denoise_params_default(None)
    w, h = 160, 100
    c = api.Context(0)
    try:
        assert c.denoise_time_ms() == 0.0 and c.denoise_launch_ms() == []
        fb, buf, out = c.framebuffer(w, h), c.aov_buffer(w, h), c.framebuffer(w, h)

        def call(ctxh=c.h, fb_=fb, aov_=buf, out_=out, null_params=False, **kw):
            q = abi.DenoiseParams()
            L.crh_denoise_params_default(C.byref(q))
            q.width, q.height = w, h
            for k, v in kw.items():
                setattr(q, k, v)
            return L.crh_denoise(ctxh, None if null_params else C.byref(q), fb_, aov_, out_)
        assert call(ctxh=None) == abi.ERR_INVALID
        assert call(null_params=True) == abi.ERR_INVALID
        assert call(fb_=None) == abi.ERR_INVALID and call(aov_=None) == abi.ERR_INVALID and call(out_=None) == abi.ERR_INVALID
        assert call(width=0) == abi.ERR_INVALID and call(height=-3) == abi.ERR_INVALID
        assert call(iterations=-1) == abi.ERR_INVALID and call(iterations=9) == abi.ERR_INVALID
        for field in ("sigma_normal", "sigma_depth", "sigma_color"):
            for bad in (0.0, -1.0, float("nan"), float("inf")):
                assert call(**{field: bad}) == abi.ERR_INVALID, (field, bad)
        assert call(out_=buf) == abi.ERR_INVALID                                     # the output aliases the guides
        assert L.crh_denoise_time_ms(c.h, None) == abi.ERR_INVALID and L.crh_denoise_time_ms(None, C.byref(C.c_float())) == abi.ERR_INVALID
        with pytest.raises(TypeError):
            c.denoise(fb, buf, w, h, sigma=1.0)
        assert c.denoise_time_ms() == 0.0, "refused calls are no calls"
        # no scene is needed
        assert call() == abi.OK and call(iterations=0) == abi.OK and call(iterations=8, out_=fb) == abi.OK
        assert c.denoise_time_ms() > 0.0 and len(c.denoise_launch_ms()) == 9
        assert not c.download(out, w, h).any(), "a black frame stays black"
        # the render path's counters, time and kernel name are the render's after a denoise
        c.upload(api.Scene(golden_blob("glowmetal")))
        c.reset_counters()
        c.render_region(fb, w, h, 2, 3)
        c.render_aov(buf, w, h, 2)
        frame = c.download(fb, w, h)
        before = (c.counters(), c.kernel_time_ms(), c.last_kernel_name())
        c.denoise(fb, buf, w, h, out=out)
        img = c.download(out, w, h)
        assert (c.counters(), c.kernel_time_ms(), c.last_kernel_name()) == before
        launches = c.denoise_launch_ms()
        assert len(launches) == 6 and all(t > 0.0 for t in launches) and abs(c.denoise_time_ms() - sum(launches)) <= 1e-4 * sum(launches)
        assert img.any() and (bits(img) != bits(frame)).any() and np.array_equal(bits(c.download(fb, w, h)), bits(frame))
    finally:
        c.close()


# ---- 6. the drop-in program ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dropin_program_writes_the_denoised_frame(pkg, ctx, manifest, golden_blob, tmp_path):
    """c-ray-hip with CRAY_HIP_DENOISE=3: the dump equals Context.denoise of the same frame and guides, exactly one more image stands beside the frame, and
    the frame's own image is the one of the run without the variable."""
    if not dropin_paths()[2]:
        pytest.skip("c-ray-hip or the asset overlay is not built (needs the reference's sources at build time)")
    m = manifest["cfg1_scene"]
    w, h, s = m["width"], m["height"], m["samples"]
    env = dict(dropin_env(), CRH_DUMP_F32=str(tmp_path / "frame.f32"))
    plain_files, _ = run_dropin(manifest, tmp_path, env)
    plain = sorted(f for f in plain_files if f.endswith(".bmp"))
    assert len(plain) == 1, plain
    plain_bmp = plain_files[plain[0]]
    all_files, _ = run_dropin(manifest, tmp_path, dict(env, CRAY_HIP_DENOISE="3", CRH_DUMP_DENOISED_F32=str(tmp_path / "denoised.f32")))
    assert all_files["frame.f32"] == plain_files["frame.f32"], "the frame itself is untouched"
    frame = np.frombuffer(all_files["frame.f32"], np.float32).reshape(h, w, 3)
    got = np.frombuffer(all_files["denoised.f32"], np.float32).reshape(h, w, 3)
    # the guides the program renders: min(16, sampleCount) passes of sampleCount
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    buf = ctx.aov_buffer(w, h)
    ctx.render_aov(buf, w, h, s, pass_count=min(16, s))
    aov = ctx.download_aov(buf, w, h)
    assert aov[..., 7].any()
    want = gpu_denoise(pkg, ctx, frame, aov, iterations=3)
    assert_bit_equal(got, want, "drop-in")
    assert (bits(got) != bits(frame)).any()
    files = sorted(f for f in all_files if f.endswith(".bmp"))
    stem = plain[0][:-len("_0000.bmp")]
    assert files == sorted(plain + [f"{stem}_denoised_0000.bmp"]), files
    assert all_files[plain[0]] == plain_bmp, "the frame's image changed"
    data = all_files[f"{stem}_denoised_0000.bmp"]
    assert data[:2] == b"BM" and int.from_bytes(data[18:22], "little") == w and abs(int.from_bytes(data[22:26], "little", signed=True)) == h
    assert data != plain_bmp


# ---- 7. the CPU tier ---------------------------------------------------------------------------------------------------------------------------------
def test_denoise_kernels_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the kernel emulation (tests/emu/libcray_hip_emu.so: the denoise kernels and crh_denoise
    compiled unmodified on the HIP-on-CPU shim) — every one of them runs and passes there, none skipped (the drop-in test where the drop-in program is built)."""
    run_gpu_tests_on_emulation(__file__, 16, passed_without_dropin=15)
