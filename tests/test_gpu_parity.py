"""GPU tier: the HIP path, called through the C-ABI (libcray_hip.so), against the oracle.

The bar (stated once, used everywhere below): BIT-EXACT.
  * traversal: fp32 add/mul/fma/div/sqrt are IEEE on both sides, so crh_trace_rays returns the oracle's records bit for
    bit (instance, polygon, distance, hit point, normal, uv, per-ray node / triangle test counts).
  * images: the libm functions of the path (sinf, cosf, tanf, powf, logf, log10f, atan2f, acosf, asinf) are restated in
    c-ray_amd/csrc/exact_math.h with the bits of the reference's host libm (glibc 2.35, x86-64 FMA variants; checked over all
    2^32 inputs by tests/test_exact_math.py), so the device frame equals the reference's float buffer exactly — every fixture,
    including statues.json, whose own chaos (transparent plane re-hit at t ~ 0) makes the SAME reference sources differ from
    themselves in 42 % of the pixels when only FMA contraction changes. Ray counts are equal; node-test counts are equal
    unless a zero-component ray took the exact-slab path (fewer visits).
"""
import numpy as np
import pytest

from conftest import BIG_CASES, built_blob, camera_rays, image_stats, kernel_forms, resize_camera
from support import ctx, dropin_env, dropin_paths  # noqa: F401 (ctx: the module-scoped device context)

pytestmark = pytest.mark.gpu
CASES = ["cfg1_scene", "alphanode", "fence", "glowmetal", "refraction", "uvsphere", "texwrap"]
# ... and an edge scene for the frames: one bsdf parameter at an edge value per sphere (tests/test_bsdf_edges.py; its frame holds no NaN — bsdfedges_b's does, and is
# compared there, a NaN equal to a NaN of any payload)
IMAGE_CASES = CASES + ["bsdfedges_a"]


def gpu_render(pkg, ctx, blob, w, h, s, b, **kw):
    scene = pkg.api.Scene(blob)
    ctx.upload(scene)
    fb = ctx.framebuffer(w, h)
    ctx.reset_counters()
    ctx.render_region(fb, w, h, s, b, **kw)
    img = ctx.download(fb, w, h)
    return img, ctx.counters(), fb


@pytest.mark.parametrize("name", CASES)
def test_trace_rays_bit_exact(name, pkg, ctx, oracle, golden_blob):
    blob = golden_blob(name)
    ctx.upload(pkg.api.Scene(blob))
    oscene = oracle.OracleScene(blob)
    rays = camera_rays(oscene.desc, 100000, 5)
    hg, ho = ctx.trace_rays(rays), oracle.trace_rays(oscene, rays)
    for f in ("inst", "poly", "distance", "point", "normal", "node_tests", "tri_tests", "material"):
        assert np.array_equal(hg[f], ho[f]), f"{name}: {f} differs in {(hg[f] != ho[f]).sum()} records"
    assert np.array_equal(hg["uv"], ho["uv"])
    assert (ho["inst"] >= 0).sum() > 500


@pytest.mark.parametrize("name", IMAGE_CASES)
def test_image_parity_vs_reference(name, pkg, ctx, oracle, manifest, golden_blob, golden_ref):
    m = manifest[name]
    img, cnt, _ = gpu_render(pkg, ctx, golden_blob(name), m["width"], m["height"], m["samples"], m["bounces"])
    ref = golden_ref(name)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (name, image_stats(img, ref))
    assert cnt["paths"] == m["width"] * m["height"] * m["samples"]
    assert cnt["rays"] == m["rays"], (cnt["rays"], m["rays"])
    assert 0.98 * m["node_tests"] <= cnt["node_tests"] <= m["node_tests"]


@pytest.mark.parametrize("name", ["cfg3_venus", "cfg4_statues", "soup_1m"])
def test_trace_rays_bit_exact_on_baseline_configs(name, pkg, ctx, oracle):
    """BASELINE.json configs[2..4] at full scene size (deep BLAS; 55-instance TLAS; 1 M-triangle soup without normals):
    getClosestIsect records and per-ray node / triangle test counts equal the oracle's bit for bit."""
    blob = built_blob(name)
    ctx.upload(pkg.api.Scene(blob))
    oscene = oracle.OracleScene(blob)
    rays = camera_rays(oscene.desc, 50000, 7)
    hg, ho = ctx.trace_rays(rays), oracle.trace_rays(oscene, rays)
    for f in ("inst", "poly", "distance", "point", "normal", "node_tests", "tri_tests", "material"):
        assert np.array_equal(hg[f], ho[f]), f"{name}: {f} differs in {(hg[f] != ho[f]).sum()} records"
    assert np.array_equal(hg["uv"].view(np.uint32), ho["uv"].view(np.uint32)), f"{name}: uv differs in {(hg['uv'].view(np.uint32) != ho['uv'].view(np.uint32)).sum()} words"
    assert (ho["inst"] >= 0).sum() > 500


@pytest.mark.parametrize("name", BIG_CASES)
def test_image_parity_on_baseline_configs_reduced_frame(name, pkg, ctx, manifest, golden_ref):
    """BASELINE.json configs[1..4] at 320x180, 4 spp, the configs' own bounce limits: the real reference's frame (c-ray-ref-strict)
    bit for bit, ray counts equal. (The manifest also records each scene's chaos floor — how far the SAME reference sources land from
    themselves when only FMA contraction changes: 42 % of the pixels of statues.json — which is why anything short of identical
    libm bits cannot meet a pixel gate there.)"""
    m = manifest[name]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    scene = resize_camera(pkg.api.Scene(built_blob(m["built_blob"])), w, h)
    ctx.upload(scene)
    fb = ctx.framebuffer(w, h)
    ctx.reset_counters()
    ctx.render_region(fb, w, h, s, b)
    img, cnt = ctx.download(fb, w, h), ctx.counters()
    ref = golden_ref(name)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (name, image_stats(img, ref), m["floor"])
    assert cnt["paths"] == w * h * s and cnt["rays"] == m["rays"]
    assert 0.98 * m["node_tests"] <= cnt["node_tests"] <= m["node_tests"]          # (the default: zero-component rays take the exact slab test and visit fewer nodes)
    # ... and with the reference's own arithmetic on those rays (CRH_OPT_RENDER_SLABS = LITERAL: bvh.c:326-352 NaN for NaN) the walk is the reference's node for node
    ctx.set_option(pkg.abi.OPT_RENDER_SLABS, pkg.abi.TRACE_SLABS_LITERAL)
    try:
        ctx.clear(fb, w, h); ctx.reset_counters()
        ctx.render_region(fb, w, h, s, b)
        img, cnt = ctx.download(fb, w, h), ctx.counters()
    finally:
        ctx.set_option(pkg.abi.OPT_RENDER_SLABS, pkg.abi.TRACE_SLABS_EXACT)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (name, "literal slabs", image_stats(img, ref))
    assert cnt["rays"] == m["rays"] and cnt["node_tests"] == m["node_tests"], (name, cnt["node_tests"], m["node_tests"])


def test_sampler_key_wraps_at_4k_2048spp(pkg, ctx, oracle):
    """configs[3] is 3840x2160 at 2048 spp: pixelIndex * maxPasses + pass exceeds 2^32 for every row above y = 546 and the
    reference's 32-bit key wraps (sampler.c:42). Two passes of a strip up there, seeded with maxPasses = 2048, against the oracle."""
    blob = built_blob("cfg4_statues")
    w, h, b = 3840, 2160, 30
    region = (1800, 1200, 1928, 1216)
    ctx.upload(pkg.api.Scene(blob))
    fb = ctx.framebuffer(w, h)
    ctx.reset_counters()
    ctx.render_region(fb, w, h, 2048, b, first_pass=0, pass_count=2, region=region)
    img, cnt = ctx.download(fb, w, h), ctx.counters()
    oscene = oracle.OracleScene(blob)
    ref = np.zeros((h, w, 3), np.float32)
    _, ocnt = oracle.render(oscene, w, h, 2048, b, region=region, first_pass=0, pass_count=2, fb=ref)
    x0, y0, x1, y1 = region
    a, r = img[h - y1:h - y0, x0:x1], ref[h - y1:h - y0, x0:x1]
    assert (region[1] * w + region[0]) * 2048 > 2 ** 32
    assert np.array_equal(a, r), float((np.abs(a - r).max(axis=2) == 0.0).mean())      # with any other seeds < 0.1 % of the pixels agree
    assert cnt["rays"] == ocnt["rays"]
    mask = np.ones((h, w), bool); mask[h - y1:h - y0, x0:x1] = False
    assert not img[mask].any()


def test_cfg3_full_width_strip_seeded_for_1024_passes(pkg, ctx, oracle):
    """configs[2] (venus.json, 1920x1080, 1024 spp, 32 bounces) at its REAL frame size and sampler seeds: a full-width 8-row strip, the first two of maxPasses = 1024
    passes, against the oracle float for float (round 5: until then the driver-run suite held this config at 320x180 only; the seed of a (pixel, pass) depends on
    the frame's width and on maxPasses, sampler.c:42)."""
    blob = built_blob("cfg3_venus")
    w, h, b = 1920, 1080, 32
    region = (0, 500, w, 508)
    ctx.upload(pkg.api.Scene(blob))
    fb = ctx.framebuffer(w, h)
    ctx.reset_counters()
    ctx.render_region(fb, w, h, 1024, b, first_pass=0, pass_count=2, region=region)
    img, cnt = ctx.download(fb, w, h), ctx.counters()
    oscene = oracle.OracleScene(blob)
    ref = np.zeros((h, w, 3), np.float32)
    _, ocnt = oracle.render(oscene, w, h, 1024, b, region=region, first_pass=0, pass_count=2, fb=ref)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), int((img != ref).sum())
    assert cnt["rays"] == ocnt["rays"] and cnt["rays"] > 2 * w * 8
    assert img[h - 508:h - 500].any()


def test_cfg4_rank_share_strips_at_full_size(pkg, ctx, oracle):
    """The multi-GPU share at configs[3]'s real size, pixel for pixel (round 5): rank 3 of 8's strips — 4-row strips, strip i to rank i mod 8 (render.py: owned_tiles, the C
    host's share.h) — of statues.json at 3840x2160, handed to crh_render_tiles as that rank would hand them; two of them (8 full-width rows, the first two of 2048
    passes) are held against the oracle float for float, and no pixel outside the rank's share is touched."""
    render = pkg.render
    blob = built_blob("cfg4_statues")
    w, h, b = 3840, 2160, 30
    mine = render.owned_tiles(w, h, 64, 64, 0, 3, 8)
    assert len(mine) == (h // render.STRIP_ROWS) // 8 + (1 if 3 < (h // render.STRIP_ROWS) % 8 else 0) and all(t[0] == 0 and t[2] == w for t in mine)
    picked = [mine[len(mine) // 2], mine[len(mine) // 2 + 1]]          # two strips of the share, 32 rows apart
    ctx.upload(pkg.api.Scene(blob))
    fb = ctx.framebuffer(w, h)
    ctx.reset_counters()
    ctx.render_tiles(fb, w, h, 2048, b, picked, first_pass=0, pass_count=2)
    img, cnt = ctx.download(fb, w, h), ctx.counters()
    oscene = oracle.OracleScene(blob)
    ref = np.zeros((h, w, 3), np.float32)
    rays = 0
    for t in picked:
        _, ocnt = oracle.render(oscene, w, h, 2048, b, region=t, first_pass=0, pass_count=2, fb=ref)
        rays += ocnt["rays"]
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), int((img != ref).sum())
    assert cnt["rays"] == rays
    rows = np.zeros(h, bool)
    for (_, y0, _, y1) in picked:
        rows[h - y1:h - y0] = True
    assert img[rows].any() and not img[~rows].any()
    # ... and the whole share is a disjoint cover with the other ranks' (host logic; the gloo tests assemble the frame)
    seen = np.zeros(h, np.int32)
    for r in range(8):
        for (_, y0, _, y1) in render.owned_tiles(w, h, 64, 64, 0, r, 8):
            seen[y0:y1] += 1
    assert (seen == 1).all()


def test_shade_class_batches_change_nothing(pkg, ctx, manifest, golden_blob, golden_ref):
    """CRH_OPT_SHADE_SORT: scenes with at least that many shade classes (instances whose hits run the same surface-shader code path) shade their hits in batches
    of few classes; which hits share a batch is pure scheduling. hdr.json at 320x180 (six classes) and the node zoo (dozens of graphs, the
    programs + volumes kernel variant): every batch threshold gives the reference's frame bit for bit."""
    for name in ("cfg2_hdr_small", "nodezoo"):
        m = manifest[name]
        w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
        ref = golden_ref(name)
        if "built_blob" in m:
            ctx.upload(resize_camera(pkg.api.Scene(built_blob(m["built_blob"])), w, h))
        else:
            ctx.upload(pkg.api.Scene(golden_blob(m.get("blob", name))))
        fb = ctx.framebuffer(w, h)
        for sort_from, shade_min in ((4, 48), (2, 1), (1, 17), (4, 64), (3, 128), (0, 48)):        # CRH_OPT_SHADE_SORT (0 = the default: no batches by class)
            ctx.set_option(pkg.abi.OPT_SHADE_SORT, sort_from)
            ctx.set_sched(70, 160, 120, 16, shade_min=shade_min)
            ctx.clear(fb, w, h)
            ctx.render_region(fb, w, h, s, b)
            assert np.array_equal(ctx.download(fb, w, h), ref), (name, sort_from, shade_min)
    ctx.set_option(pkg.abi.OPT_SHADE_SORT, 0)
    ctx.set_sched(70, 160, 120, 16)


def test_dispatch_decompositions_are_bit_identical(pkg, ctx, manifest, golden_blob):
    """Tile lists, region splits, pass splits and every block/chunk shape give the same frame bit for bit
    (a pixel's passes are folded in order whatever the schedule)."""
    m = manifest["refraction"]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    full, cnt_full, fb = gpu_render(pkg, ctx, golden_blob("refraction"), w, h, s, b)
    # two pass ranges
    ctx.clear(fb, w, h)
    ctx.render_region(fb, w, h, s, b, first_pass=0, pass_count=1)
    ctx.render_region(fb, w, h, s, b, first_pass=1)
    assert np.array_equal(ctx.download(fb, w, h), full)
    # the reference's tile list, interleaved over 3 "ranks", each in one multi-tile dispatch
    tiles = pkg.tiles.quantize_image(w, h, 32, 32, pkg.tiles.ORDER_FROM_MIDDLE)
    ctx.clear(fb, w, h)
    ctx.reset_counters()
    for r in range(3):
        ctx.render_tiles(fb, w, h, s, b, pkg.tiles.tiles_for_rank(tiles, r, 3))
    assert np.array_equal(ctx.download(fb, w, h), full)
    assert ctx.counters() == cnt_full
    # schedule knobs
    for items, chunk in ((64, 1), (4096, 2), (1 << 16, 64)):
        ctx.set_option(pkg.abi.OPT_UNIT_ITEMS, items)
        ctx.set_option(pkg.abi.OPT_PASS_CHUNK, chunk)
        ctx.clear(fb, w, h)
        ctx.render_region(fb, w, h, s, b)
        assert np.array_equal(ctx.download(fb, w, h), full), (items, chunk)
    ctx.set_option(pkg.abi.OPT_UNIT_ITEMS, 1024)
    ctx.set_option(pkg.abi.OPT_PASS_CHUNK, 64)
    # wave scheduler: which step kind runs when changes nothing a path computes
    for sched in ((1, 1, 1, 1, 0, 8, 65, 65, 0, 65), (400, 10, 10, 64, 64, 1, 1, 1, 0, 1), (10, 10, 400, 8, 192, 4, 20, 40, 0, 7), (70, 160, 120, 16, 160, 4, 12, 12, 0, 64)):          # (the last field: retire / refill inside node runs)
        ctx.set_sched(*sched)
        ctx.clear(fb, w, h)
        ctx.render_region(fb, w, h, s, b)
        assert np.array_equal(ctx.download(fb, w, h), full), sched
    ctx.set_sched(70, 160, 120, 16)
    # tapered units: how much of the dispatch ends the work queue as quarter-size blocks (incl. a row-split of the single tile)
    for tail in (0, 50, 7):
        ctx.set_option(pkg.abi.OPT_TAIL_PERCENT, tail)
        ctx.clear(fb, w, h)
        ctx.reset_counters()
        ctx.render_region(fb, w, h, s, b)
        assert np.array_equal(ctx.download(fb, w, h), full), tail
        assert ctx.counters() == cnt_full
    ctx.set_option(pkg.abi.OPT_TAIL_PERCENT, 16)
    # both register-budget variants and both counter levels compute the same frame
    for wps, level in ((1, 2), (1, 1), (4, 1)):
        ctx.set_option(pkg.abi.OPT_WAVES_PER_SIMD, wps)
        ctx.set_option(pkg.abi.OPT_COUNTER_LEVEL, level)
        ctx.clear(fb, w, h)
        ctx.reset_counters()
        ctx.render_region(fb, w, h, s, b)
        assert np.array_equal(ctx.download(fb, w, h), full), (wps, level)
        assert ctx.counters()["rays"] == cnt_full["rays"]
    ctx.set_option(pkg.abi.OPT_WAVES_PER_SIMD, 4)
    ctx.set_option(pkg.abi.OPT_COUNTER_LEVEL, 2)


def test_streaming_form_is_bit_identical(pkg, ctx, manifest, golden_blob, golden_ref):
    """CRH_KERNEL_STREAM (csrc/pathtrace_stream.h: walk / shade + refill / fold kernels over two path pools) renders the reference's frame bit for bit, with the rolling
    kernel's counters, whatever the pool size (seven cohorts: chunks of one pass; one cohort and 24 passes of a small region: dozens of iterations and a ring of sample
    slabs that turns over), for pass ranges and tile lists; dispatches it cannot serve (volumes: a sampler draw inside the walk) are rendered by the rolling kernel."""
    abi = pkg.abi

    def streamed(fb, w, h, s, b, **kw):
        ctx.clear(fb, w, h); ctx.reset_counters()
        ctx.render_region(fb, w, h, s, b, **kw)
        assert ctx.last_kernel_name().startswith("k_stream"), ctx.last_kernel_name()
        return ctx.download(fb, w, h), ctx.counters()
    try:
        # the fixture's frame, two pool sizes
        m = manifest["cfg1_scene"]
        w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
        ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_ROLL)
        img, cnt, fb = gpu_render(pkg, ctx, golden_blob("cfg1_scene"), w, h, s, b)
        assert np.array_equal(img, golden_ref("cfg1_scene"))
        region = (16, 24, 64, 56)          # 48 x 32 pixels, 24 passes: more chunks than the ring has slabs when the pool is one cohort
        ctx.clear(fb, w, h); ctx.reset_counters()
        ctx.render_region(fb, w, h, 24, b, region=region)
        small, small_cnt = ctx.download(fb, w, h), ctx.counters()
        ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_STREAM)
        for cohorts in (16384, 7):
            ctx.set_option(abi.OPT_STREAM_COHORTS, cohorts)
            got, got_cnt = streamed(fb, w, h, s, b)
            assert np.array_equal(got, img) and got_cnt == cnt, cohorts
        ctx.set_option(abi.OPT_STREAM_COHORTS, 1)
        got, got_cnt = streamed(fb, w, h, 24, b, region=region)
        assert np.array_equal(got, small) and got_cnt == small_cnt
        # pass ranges and the reference's tile list dealt over three "ranks"; counter level 1 (the timed instantiations)
        m = manifest["refraction"]
        w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
        ref = golden_ref("refraction")
        ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_ROLL)
        img, cnt, fb = gpu_render(pkg, ctx, golden_blob("refraction"), w, h, s, b)
        assert np.array_equal(img, ref)
        ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_STREAM)
        ctx.set_option(abi.OPT_STREAM_COHORTS, 3)
        ctx.clear(fb, w, h)
        ctx.render_region(fb, w, h, s, b, first_pass=0, pass_count=1)
        ctx.render_region(fb, w, h, s, b, first_pass=1)
        assert np.array_equal(ctx.download(fb, w, h), ref)
        ctx.set_option(abi.OPT_STREAM_COHORTS, 16384)
        tiles = pkg.tiles.quantize_image(w, h, 32, 32, pkg.tiles.ORDER_FROM_MIDDLE)
        ctx.clear(fb, w, h); ctx.reset_counters()
        for r in range(3):
            ctx.render_tiles(fb, w, h, s, b, pkg.tiles.tiles_for_rank(tiles, r, 3))
        assert np.array_equal(ctx.download(fb, w, h), ref)
        assert ctx.counters() == cnt
        ctx.set_option(abi.OPT_COUNTER_LEVEL, 1)
        got, got_cnt = streamed(fb, w, h, s, b)
        assert np.array_equal(got, ref) and got_cnt["rays"] == cnt["rays"] and got_cnt["paths"] == cnt["paths"]
        ctx.set_option(abi.OPT_COUNTER_LEVEL, 2)
        # a scene with volumes: the option stays set, the rolling kernel renders
        m = manifest["volumes"]
        img, _, _ = gpu_render(pkg, ctx, golden_blob("volumes"), m["width"], m["height"], m["samples"], m["bounces"])
        assert ctx.last_kernel_name().startswith("k_pathtrace_roll"), ctx.last_kernel_name()
        assert np.array_equal(img, golden_ref("volumes"))
    finally:
        ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_ROLL)
        ctx.set_option(abi.OPT_STREAM_COHORTS, 16384)
        ctx.set_option(abi.OPT_COUNTER_LEVEL, 2)


def test_rolling_and_one_unit_at_a_time_kernels_are_bit_identical(pkg, ctx, manifest, golden_blob):
    """CRH_OPT_KERNEL: the default form keeps up to four work units open per wave (k_pathtrace_roll), CRH_KERNEL_WAVE works one unit at a time (the default
    until round 3). Same per-path operations, so: the same frame and the same counters — for default and tiny units, one-pass chunks, ragged tiles split
    over two dispatches, both counter levels."""
    abi = pkg.abi
    ref_kernel = abi.KERNEL_WAVE if abi.KERNEL_WAVE in kernel_forms(pkg, ctx) else abi.KERNEL_ROLL      # (product library: the rolling kernel at its default settings; the forms meet in the emulation tier)
    try:
        for name in ("refraction", "glowmetal", "cfg1_scene", "fence"):
            m = manifest[name]
            w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
            ctx.set_option(abi.OPT_KERNEL, ref_kernel)
            full, cnt_full, fb = gpu_render(pkg, ctx, golden_blob(name), w, h, s, b)
            ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_ROLL)
            for items, chunk in ((2048, 64), (64, 1), (256, 2)):
                ctx.set_option(abi.OPT_UNIT_ITEMS, items)
                ctx.set_option(abi.OPT_PASS_CHUNK, chunk)
                for level in (2, 1):
                    ctx.set_option(abi.OPT_COUNTER_LEVEL, level)
                    ctx.clear(fb, w, h)
                    ctx.reset_counters()
                    ctx.render_region(fb, w, h, s, b)
                    assert np.array_equal(ctx.download(fb, w, h), full), (name, items, chunk, level)
                    got = ctx.counters()
                    assert got["rays"] == cnt_full["rays"] and got["paths"] == cnt_full["paths"]
                    if level == 2:
                        assert got == cnt_full, (name, items, chunk)
            ctx.set_option(abi.OPT_COUNTER_LEVEL, 2)
            ctx.clear(fb, w, h)
            ctx.render_tiles(fb, w, h, s, b, [(0, 0, w - 1, h // 3), (0, h // 3, w - 1, h), (w - 1, 0, w, h)], first_pass=0, pass_count=1)
            ctx.render_tiles(fb, w, h, s, b, [(0, 0, w, h)], first_pass=1)
            assert np.array_equal(ctx.download(fb, w, h), full), name
    finally:
        ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_ROLL)
        ctx.set_option(abi.OPT_COUNTER_LEVEL, 2)
        ctx.set_option(abi.OPT_UNIT_ITEMS, 2048)
        ctx.set_option(abi.OPT_PASS_CHUNK, 64)


def test_split_pixels_fold_in_pass_order(pkg, ctx, manifest, golden_blob):
    """CRH_OPT_TAIL_SPLIT: the rolling kernel's work queue ends with 64-path units — from 128 passes per dispatch on these are pass SEGMENTS of single pixels, traced
    by whichever waves pull them, their samples staged per pixel and folded behind the kernel (k_fold_deferred). The frame is the one-unit-at-a-time kernel's
    bit for bit: a ragged last segment (160 = 64 + 64 + 32), pass ranges (the second dispatch continues the running mean of the first; 30 passes are not split),
    tile lists with ragged edges, every number of split units per wave, both counter levels; with fewer passes the last units are small blocks (no pixel split)."""
    abi = pkg.abi
    ref_kernel = abi.KERNEL_WAVE if abi.KERNEL_WAVE in kernel_forms(pkg, ctx) else abi.KERNEL_ROLL      # (product library: the rolling kernel without split units)
    try:
        for name, w, h, s in (("refraction", 48, 30, 160), ("glowmetal", 37, 19, 257), ("cfg1_scene", 64, 40, 24)):
            b = manifest[name]["bounces"]
            ctx.set_option(abi.OPT_KERNEL, ref_kernel)
            ctx.set_option(abi.OPT_TAIL_SPLIT, 0)
            full, cnt_full, fb = gpu_render(pkg, ctx, golden_blob(name), w, h, s, b)
            ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_ROLL)
            for split in (4, 0, 1, 64):
                for level in (2, 1):
                    ctx.set_option(abi.OPT_TAIL_SPLIT, split)
                    ctx.set_option(abi.OPT_COUNTER_LEVEL, level)
                    ctx.clear(fb, w, h)
                    ctx.reset_counters()
                    ctx.render_region(fb, w, h, s, b)
                    assert np.array_equal(ctx.download(fb, w, h), full), (name, split, level)
                    got = ctx.counters()
                    assert got["rays"] == cnt_full["rays"] and got["paths"] == cnt_full["paths"], (name, split, level)
            ctx.set_option(abi.OPT_COUNTER_LEVEL, 2)
            ctx.set_option(abi.OPT_TAIL_SPLIT, 8)
            ctx.clear(fb, w, h)
            first = max(1, s - 30)
            ctx.render_tiles(fb, w, h, s, b, [(0, 0, w - 1, h // 3), (0, h // 3, w - 1, h), (w - 1, 0, w, h)], first_pass=0, pass_count=first)
            ctx.render_tiles(fb, w, h, s, b, [(0, 0, w, h)], first_pass=first)
            assert np.array_equal(ctx.download(fb, w, h), full), name
            tiles = pkg.tiles.quantize_image(w, h, 16, 16, pkg.tiles.ORDER_FROM_MIDDLE)
            ctx.clear(fb, w, h)
            for r in range(3):
                ctx.render_tiles(fb, w, h, s, b, pkg.tiles.tiles_for_rank(tiles, r, 3))
            assert np.array_equal(ctx.download(fb, w, h), full), name
    finally:
        ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_ROLL)
        ctx.set_option(abi.OPT_COUNTER_LEVEL, 2)
        ctx.set_option(abi.OPT_TAIL_SPLIT, abi.TAIL_SPLIT_DEFAULT)


def test_workgroup_kernel_is_bit_identical_to_the_wave_kernel(pkg, ctx, manifest, golden_blob):
    """CRH_OPT_KERNEL: the workgroup-cooperative form (walker / shader roles, shared path table, LDS lock) runs the same per-path
    operations as the per-wave machine — same frame, same counters, for every scheduler setting incl. the degenerate ones (never
    linger / always linger, drain at once / never, no drainers, partial batches of 1, tables of 64 paths), both samplers, a scene with
    node programs, multi-chunk passes and ragged tiles."""
    abi = pkg.abi
    if abi.KERNEL_WG not in kernel_forms(pkg, ctx):
        with pytest.raises(pkg.api.CrhError) as e:          # the product library says so instead of launching something else
            ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_WG)
        assert e.value.code == abi.ERR_UNSUPPORTED and "CRH_WITH_ALT_KERNELS" in str(e.value)
        pytest.skip("the product library holds k_pathtrace_roll only (round 4); this comparison runs in the emulation tier (tests/test_kernel_emu.py)")
    scheds = [(8, 192, 1, 16, 32, 768), (0, 1, 4, 1, 1, 64), (255, 4095, 0, 64, 64, 960), (3, 64, 2, 8, 16, 256)]
    try:
        for name in ("refraction", "glowmetal", "cfg1_scene"):
            m = manifest[name]
            w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
            ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_WAVE)
            full, cnt_full, fb = gpu_render(pkg, ctx, golden_blob(name), w, h, s, b)
            ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_WG)
            for sc in scheds:
                ctx.set_sched_wg(*sc)
                for level in (2, 1):
                    ctx.set_option(abi.OPT_COUNTER_LEVEL, level)
                    ctx.clear(fb, w, h)
                    ctx.reset_counters()
                    ctx.render_region(fb, w, h, s, b)
                    assert np.array_equal(ctx.download(fb, w, h), full), (name, sc, level)
                    got = ctx.counters()
                    assert got["rays"] == cnt_full["rays"] and got["paths"] == cnt_full["paths"]
                    if level == 2:
                        assert got == cnt_full, (name, sc)
            ctx.set_sched_wg()
            ctx.set_option(abi.OPT_COUNTER_LEVEL, 2)
            # ragged tiles, pass splits and small units through the workgroup kernel
            ctx.set_option(abi.OPT_UNIT_ITEMS, 64)
            ctx.set_option(abi.OPT_PASS_CHUNK, 1)
            ctx.clear(fb, w, h)
            ctx.render_tiles(fb, w, h, s, b, [(0, 0, w - 1, h // 3), (0, h // 3, w - 1, h), (w - 1, 0, w, h)], first_pass=0, pass_count=1)
            ctx.render_tiles(fb, w, h, s, b, [(0, 0, w, h)], first_pass=1)
            assert np.array_equal(ctx.download(fb, w, h), full), name
            ctx.set_option(abi.OPT_UNIT_ITEMS, 1024)
            ctx.set_option(abi.OPT_PASS_CHUNK, 64)
        # Halton sampler (interactive mode)
        m = manifest["cfg1_scene_iterative"]
        w, h, n, b = m["width"], m["height"], m["samples"], m["bounces"]
        ctx.upload(pkg.api.Scene(golden_blob(m["blob"])))
        fb = ctx.framebuffer(w, h)
        ctx.set_option(abi.OPT_SAMPLER, abi.SAMPLER_HALTON)
        imgs = []
        for kern in (abi.KERNEL_WAVE, abi.KERNEL_WG, abi.KERNEL_ROLL):
            ctx.set_option(abi.OPT_KERNEL, kern)
            ctx.clear(fb, w, h)
            ctx.render_region(fb, w, h, n, b, pass_count=m["passes"])
            imgs.append(ctx.download(fb, w, h))
        assert np.array_equal(imgs[0], imgs[1]) and np.array_equal(imgs[0], imgs[2])
    finally:
        ctx.set_option(abi.OPT_SAMPLER, abi.SAMPLER_RANDOM)
        ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_ROLL)
        ctx.set_option(abi.OPT_COUNTER_LEVEL, 2)
        ctx.set_option(abi.OPT_UNIT_ITEMS, 2048)
        ctx.set_option(abi.OPT_PASS_CHUNK, 64)
        ctx.set_sched_wg()


def test_zero_component_rays(pkg, ctx, oracle, golden_blob):
    blob = golden_blob("cfg1_scene")
    ctx.upload(pkg.api.Scene(blob))
    oscene = oracle.OracleScene(blob)
    rays = camera_rays(oscene.desc, 3000, 11)
    rays[0::3, 3] = 0.0
    rays[1::3, 4] = 0.0
    rays[2::3, 5] = 0.0
    ho = oracle.trace_rays(oscene, rays)
    # default (CRH_TRACE_SLABS_LITERAL): the reference's NaN slab arithmetic followed literally — its record AND its visit counts, ray for ray
    hg = ctx.trace_rays(rays)
    for f in ("inst", "poly", "distance", "point", "normal", "material", "node_tests", "tri_tests"):
        assert np.array_equal(hg[f], ho[f]), f
    # what the render kernels do with such rays (exact slabs): the same hits on these rays, never more node visits — far fewer
    ctx.set_option(pkg.abi.OPT_TRACE_SLABS, pkg.abi.TRACE_SLABS_EXACT)
    try:
        hx = ctx.trace_rays(rays)
    finally:
        ctx.set_option(pkg.abi.OPT_TRACE_SLABS, pkg.abi.TRACE_SLABS_LITERAL)
    for f in ("inst", "poly", "distance", "point", "normal", "material"):
        assert np.array_equal(hx[f], ho[f]), f
    assert (hx["node_tests"] <= ho["node_tests"]).all() and hx["node_tests"].sum() < 0.25 * ho["node_tests"].sum()


def test_rendered_frame_of_zero_component_rays_literal_slabs(pkg, ctx, oracle, golden_blob):
    """CRH_OPT_RENDER_SLABS = LITERAL puts degenerate rays through a RENDERED frame: with a zero-size sensor and an axis-aligned
    camera every camera ray of the frame is the same ray with two exactly-zero direction components (camera.c:66-75: pixX = pixY = 0, direction = forward),
    the case the reference's NaN slab arithmetic turns into a walk of most of the scene (bvh.c:326-352). With LITERAL the frame AND the node / triangle
    test counts equal the oracle's (which restates that arithmetic literally); the default (EXACT slabs) gives the same frame on this scene with
    far fewer node visits — the documented difference is in the visits, DESIGN.md section 5."""
    api, abi = pkg.api, pkg.abi
    blob = golden_blob("cfg1_scene")
    scene, oscene = api.Scene(blob), oracle.OracleScene(blob)
    w, h, s, b = 12, 8, 3, 4
    for d in (scene.desc, oscene.desc):
        cam = d.camera
        cam.width, cam.height = w, h
        cam.sensor[0] = cam.sensor[1] = 0.0
        cam.aperture = 0.0
        for i, v in enumerate((1.0, 0.0, 0.0)): cam.right[i] = v
        for i, v in enumerate((0.0, 1.0, 0.0)): cam.up[i] = v
        for i, v in enumerate((0.0, 0.0, 1.0)): cam.forward[i] = v
        pos = (cam.A[3], cam.A[7], cam.A[11])
        for i, v in enumerate((1.0, 0.0, 0.0, pos[0], 0.0, 1.0, 0.0, pos[1], 0.0, 0.0, 1.0, pos[2])): cam.A[i] = v       # keep the position, drop the rotation
    ray = oracle.camera_ray(oscene, 3, 4, 0, s)
    assert (np.asarray(ray[3:6]) == 0.0).sum() == 2, ray               # the oracle's camera ray IS degenerate
    ref, ocnt = oracle.render(oscene, w, h, s, b)
    ctx.upload(scene)
    fb = ctx.framebuffer(w, h)
    try:
        ctx.set_option(abi.OPT_RENDER_SLABS, abi.TRACE_SLABS_LITERAL)
        ctx.reset_counters()
        ctx.render_region(fb, w, h, s, b)
        img, cnt = ctx.download(fb, w, h), ctx.counters()
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), image_stats(img, ref)
        for k in ("rays", "paths", "node_tests", "tri_tests"):
            assert cnt[k] == ocnt[k], (k, cnt[k], ocnt[k])
        ctx.set_option(abi.OPT_RENDER_SLABS, abi.TRACE_SLABS_EXACT)
        ctx.clear(fb, w, h)
        ctx.reset_counters()
        ctx.render_region(fb, w, h, s, b)
        img2, cnt2 = ctx.download(fb, w, h), ctx.counters()
        assert np.array_equal(img2.view(np.uint32), ref.view(np.uint32)), image_stats(img2, ref)
        assert cnt2["rays"] == ocnt["rays"] and cnt2["node_tests"] < cnt["node_tests"]
    finally:
        ctx.set_option(abi.OPT_RENDER_SLABS, abi.TRACE_SLABS_EXACT)


def test_round_limit_flags_an_incomplete_frame(pkg, ctx, manifest, golden_blob):
    """A wave of the path-tracing kernel that runs out of scheduling rounds (CRH_OPT_ROUND_LIMIT; the default is hours of work) gives up instead of
    spinning on — and the dispatch SAYS so: synchronize / download return CRH_ERR_HIP "incomplete frame" (round 3's kernel left silently with CRH_OK).
    The flag is cleared by the report: the next dispatch, with the limit back at its default, renders the reference frame."""
    api, abi = pkg.api, pkg.abi
    m = manifest["glowmetal"]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    full, cnt_full, fb = gpu_render(pkg, ctx, golden_blob("glowmetal"), w, h, s, b)
    try:
        ctx.set_option(abi.OPT_ROUND_LIMIT, 40)
        ctx.clear(fb, w, h)
        ctx.render_region(fb, w, h, s, b)
        with pytest.raises(api.CrhError) as e:
            ctx.synchronize()
        assert e.value.code == abi.ERR_HIP and "incomplete frame" in str(e.value)
        ctx.render_region(fb, w, h, s, b)
        with pytest.raises(api.CrhError) as e:
            ctx.download(fb, w, h)
        assert e.value.code == abi.ERR_HIP and "incomplete frame" in str(e.value)
    finally:
        ctx.set_option(abi.OPT_ROUND_LIMIT, 2000000000)
    ctx.synchronize()                                   # reported once: clean again
    ctx.clear(fb, w, h)
    ctx.reset_counters()
    ctx.render_region(fb, w, h, s, b)
    assert np.array_equal(ctx.download(fb, w, h), full) and ctx.counters() == cnt_full
    with pytest.raises(api.CrhError):
        ctx.set_option(abi.OPT_ROUND_LIMIT, 1)


def test_srgb8_matches_oracle(pkg, ctx, oracle, manifest, golden_blob):
    m = manifest["glowmetal"]
    img, _, fb = gpu_render(pkg, ctx, golden_blob("glowmetal"), m["width"], m["height"], m["samples"], m["bounces"])
    g8 = ctx.to_srgb8(fb, m["width"], m["height"]).astype(np.int32)
    o8 = oracle.to_srgb8(img).astype(np.int32)
    assert np.array_equal(g8, o8)                                      # same powf bits: same 8-bit values
    # a multi-GPU host's previews: GPU g of n fetches only the rows of ITS 4-row strips (one strided copy); together they are the frame, and a GPU touches no other row
    w, h = m["width"], m["height"]
    full = ctx.to_srgb8(fb, w, h)
    for n in (2, 3, 8):
        frame = np.full((h, w, 3), 7, np.uint8)
        for g in range(n):
            before = frame.copy()
            ctx.strips_to_srgb8(fb, w, h, 4, g, n, frame)
            owned = np.zeros(h, bool)
            for y0 in range(g * 4, h, n * 4):
                owned[h - min(y0 + 4, h):h - y0] = True
            assert np.array_equal(frame[owned], full[owned]) and np.array_equal(frame[~owned], before[~owned]), (n, g)
        assert np.array_equal(frame, full), n
    with pytest.raises(pkg.api.CrhError):
        ctx.strips_to_srgb8(fb, w, h, 4, 2, 2, np.zeros((h, w, 3), np.uint8))


def test_upload_lifecycle_host_arrays_released_behind_a_dispatch(pkg, manifest, golden_blob, golden_ref, monkeypatch):
    """crh_scene_upload leaves the compiled host arrays to the context's janitor thread, which lets them go once a dispatch of some length has been
    launched, at the next upload, or when the context ends (round 4: freeing them inside the upload cost the drop-in 20 ms per frame). Every order
    of those events: upload - upload, upload - end, upload - dispatch - upload, and the released-at-the-first-dispatch case (CRH_JANITOR_MIN_PATHS=1,
    read at the process's first dispatch) — the same frames throughout."""
    api = pkg.api
    monkeypatch.setenv("CRH_JANITOR_MIN_PATHS", "1")
    m = manifest["glowmetal"]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    frames = []
    for order in ("upload-end", "upload-upload-render", "upload-render-upload-render"):
        c = api.Context(0)
        c.upload(api.Scene(golden_blob("glowmetal")))
        if order == "upload-end":
            c.close()
            continue
        if order == "upload-render-upload-render":
            fb0 = c.framebuffer(w, h)
            c.render_region(fb0, w, h, s, b)
            frames.append(c.download(fb0, w, h))
        c.upload(api.Scene(golden_blob("glowmetal")))
        fb = c.framebuffer(w, h)
        c.render_region(fb, w, h, s, b)
        frames.append(c.download(fb, w, h))
        c.close()
    assert len(frames) == 3 and all(np.array_equal(f, frames[0]) for f in frames[1:])
    assert np.array_equal(frames[0].view(np.uint32), golden_ref("glowmetal").view(np.uint32))


def test_upload_lifecycle_callers_arrays_poisoned_and_one_compile_for_two_contexts(pkg, manifest, golden_blob, golden_ref):
    """The lifetime contract of include/cray_hip.h (round 5): crh_scene_upload retains nothing of the caller's description — every array it points to is
    overwritten with 0xA5 right after the upload returns, and the frame is still the reference's (renderer_hip.c frees the flattened scene while the first dispatch runs).
    The same for crh_scene_compile + crh_scene_upload_compiled: ONE layout compile, two contexts that copy it, the description poisoned and the handle freed before
    either renders."""
    import ctypes as C
    api = pkg.api
    m = manifest["cfg1_scene"]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    ref = golden_ref("cfg1_scene")

    def poison(scene):
        d = scene.desc
        for ptr, count, size in ((d.nodes, d.node_count, 32), (d.prim_indices, d.prim_index_count, 4), (d.polys, d.poly_count, 40), (d.vertices, d.vertex_count, 12),
                                 (d.normals, d.normal_count, 12), (d.texcoords, d.texcoord_count, 8), (d.texture_data, d.texture_bytes, 1)):
            if int(count):
                C.memset(C.cast(ptr, C.c_void_p), 0xA5, int(count) * size)

    scene = api.Scene(golden_blob("cfg1_scene"))
    c = api.Context(0)
    c.upload(scene)
    poison(scene)
    fb = c.framebuffer(w, h)
    c.render_region(fb, w, h, s, b)
    assert np.array_equal(c.download(fb, w, h).view(np.uint32), ref.view(np.uint32))
    c.close()

    scene = api.Scene(golden_blob("cfg1_scene"))
    compiles0, uploads0 = api.upload_counts()
    compiled = api.CompiledScene(scene)
    poison(scene)
    ctxs = [api.Context(0), api.Context(0)]
    for x in ctxs:
        x.upload_compiled(compiled)
    compiled.close()
    assert api.upload_counts() == (compiles0 + 1, uploads0 + 2)
    for x in ctxs:
        fb = x.framebuffer(w, h)
        x.render_region(fb, w, h, s, b)
        assert np.array_equal(x.download(fb, w, h).view(np.uint32), ref.view(np.uint32))
        assert x.counters()["rays"] == m["rays"]
        x.close()
    # error behaviour of the two-step upload: int codes and a message, like every entry point
    import ctypes as C2
    L = api.library()
    h = C2.c_void_p()
    assert L.crh_scene_compile(None, 0, C2.byref(h)) == pkg.abi.ERR_INVALID and not h.value
    scene = api.Scene(golden_blob("cfg1_scene"))
    assert L.crh_scene_compile(scene.ptr, 7, C2.byref(h)) == pkg.abi.ERR_INVALID and b"walk" in L.crh_last_error()
    assert L.crh_scene_upload_compiled(None, None) == pkg.abi.ERR_INVALID
    L.crh_compiled_scene_free(None)          # (a no-op, like free)
    bad = pkg.abi.SceneDesc.from_buffer_copy(scene.desc)
    bad.tlas_prim_count += 1
    assert L.crh_scene_compile(C2.byref(bad), 0, C2.byref(h)) == pkg.abi.ERR_INVALID and not h.value and b"TLAS" in L.crh_last_error()
    with pytest.raises(api.CrhError):          # a scene compiled for one walk does not go to a context set to the other
        x = api.Context(0)
        x.set_option(pkg.abi.OPT_WALK, pkg.abi.WALK_WIDE4)
        try:
            x.upload_compiled(api.CompiledScene(api.Scene(golden_blob("cfg1_scene"))))
        finally:
            x.close()


def test_buffers_are_reused_and_regrown_across_entry_points(pkg, manifest, golden_blob):
    """The context owns its per-dispatch device memory (csrc/ctx_buffers.h) and keeps it from call to call: ONE context walks a small frame, a larger one — cut
    into 640 rectangles of 2 x 2 pixels, so that the render, AOV and adaptive lists each outgrow their first 4096 bytes of staging and every per-wave buffer that
    depends on the dispatch is sized again — and the small one again, and at each size calls render_tiles (pass 1, a copy for the half-sample frame, pass 2),
    render_aov, denoise, denoise_variance and adaptive_step. Every output — frame, half-sample frame, AOV buffer, both denoised frames, the tiles' errors and
    continue flags and the advanced half-sample frame — equals bit for bit what a FRESH context gives for that single call on the same inputs (device pointers
    are the device's, so the fresh context reads the walking context's buffers). Correctness of each output is the other tests' business."""
    api = pkg.api
    b = manifest["fence"]["bounces"]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
    fresh_results = {}

    def scene_at(w, h):
        return resize_camera(api.Scene(golden_blob("fence")), w, h)

    def fresh(w, h, call, upload=False):
        """call(context) on a context that has done nothing else, closed afterwards"""
        c = api.Context(0)
        try:
            if upload:
                c.upload(scene_at(w, h))
            return call(c)
        finally:
            c.close()

    walker = api.Context(0)
    try:
        for w, h, cut in ((32, 20, None), (64, 40, 2), (32, 20, None)):
            tiles = [(0, 0, w, h)] if cut is None else [(x, y, x + cut, y + cut) for y in range(0, h, cut) for x in range(0, w, cut)]
            assert cut is None or len(tiles) >= 205
            walker.upload(scene_at(w, h))
            fb, half, half0, out, out_v, aov = [walker.framebuffer(w, h) for _ in range(5)] + [walker.aov_buffer(w, h)]
            got = {}
            walker.render_tiles(fb, w, h, 2, b, tiles, first_pass=0, pass_count=1)
            walker.copy_framebuffer(fb, half, w, h)
            walker.copy_framebuffer(fb, half0, w, h)
            got["pass 1"] = walker.download(half, w, h)
            walker.render_tiles(fb, w, h, 2, b, tiles, first_pass=1, pass_count=1)
            got["frame"] = walker.download(fb, w, h)
            walker.render_aov(aov, w, h, 2, tiles=tiles)
            got["aov"] = walker.download_aov(aov, w, h)
            walker.denoise(fb, aov, w, h, out=out)
            got["denoise"] = walker.download(out, w, h)
            walker.denoise_variance(fb, half, aov, w, h, 1, 2, out=out_v)
            got["denoise_variance"] = walker.download(out_v, w, h)
            got["errors"], got["flags"] = walker.adaptive_step(fb, half, w, h, tiles, 0.05)
            got["half advanced"] = walker.download(half, w, h)
            if (w, h) not in fresh_results:          # (the stream is drained: a fresh context may read the walker's buffers)
                want = {}

                def pass1(c):
                    f = c.framebuffer(w, h)
                    c.render_tiles(f, w, h, 2, b, tiles, first_pass=0, pass_count=1)
                    return c.download(f, w, h)

                def pass2(c):
                    f = c.framebuffer(w, h)
                    c.copy_framebuffer(half0, f, w, h)
                    c.render_tiles(f, w, h, 2, b, tiles, first_pass=1, pass_count=1)
                    return c.download(f, w, h)

                def first_hits(c):
                    a = c.aov_buffer(w, h)
                    c.render_aov(a, w, h, 2, tiles=tiles)
                    return c.download_aov(a, w, h)

                def denoised(c, variance):
                    o = c.framebuffer(w, h)
                    if variance:
                        c.denoise_variance(fb, half0, aov, w, h, 1, 2, out=o)
                    else:
                        c.denoise(fb, aov, w, h, out=o)
                    return c.download(o, w, h)

                def step(c):
                    hcopy = c.framebuffer(w, h)
                    c.copy_framebuffer(half0, hcopy, w, h)
                    errors, flags = c.adaptive_step(fb, hcopy, w, h, tiles, 0.05)
                    return errors, flags, c.download(hcopy, w, h)

                want["pass 1"] = fresh(w, h, pass1, upload=True)
                want["frame"] = fresh(w, h, pass2, upload=True)
                want["aov"] = fresh(w, h, first_hits, upload=True)
                want["denoise"] = fresh(w, h, lambda c: denoised(c, False))
                want["denoise_variance"] = fresh(w, h, lambda c: denoised(c, True))
                want["errors"], want["flags"], want["half advanced"] = fresh(w, h, step)
                fresh_results[(w, h)] = want
            want = fresh_results[(w, h)]
            assert got["flags"].any() and np.isfinite(got["frame"]).all() and got["aov"][..., 7].any(), "the walk renders something and at least one tile goes on"
            for what in want:
                assert np.array_equal(bits(got[what]), bits(want[what])), (w, h, what)
    finally:
        walker.close()


def test_wide_walk_option_renders_the_fixtures(pkg, manifest, golden_blob, golden_ref):
    """CRH_OPT_WALK = CRH_WALK_WIDE4 (round 5, an experiment kept as an option; the binary walk is the contract): the 4-ary walk renders these fixtures to the
    reference's frames bit for bit — no ray of theirs meets a tie or a near tie (tools/wide_walk_study.py counts where others do) — with the same ray count, fewer
    node steps (box tests / 4 against box tests / 2), and the launch names the wide instantiation."""
    api, abi = pkg.api, pkg.abi
    for name in ("cfg1_scene", "fence", "refraction"):
        m = manifest[name]
        w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
        c = api.Context(0)
        c.set_option(abi.OPT_WALK, abi.WALK_WIDE4)
        c.upload(api.Scene(golden_blob(name)))
        fb = c.framebuffer(w, h)
        c.reset_counters()
        c.render_region(fb, w, h, s, b)
        img, cnt = c.download(fb, w, h), c.counters()
        assert "wide4" in c.last_kernel_name()
        assert np.array_equal(img.view(np.uint32), golden_ref(name).view(np.uint32)), name
        assert cnt["rays"] == m["rays"] and cnt["node_tests"] / 4 < 0.7 * m["node_tests"] / 2
        c.close()


# crh_last_kernel_name() of every instantiation a dispatch can select, written out: (form, counter level, rare features, sampler[, waves per SIMD]) -> name
KERNEL_NAMES = {
    ("roll", 1, False, 0): "k_pathtrace_roll<1,4,false,0>", ("roll", 1, False, 1): "k_pathtrace_roll<1,4,false,1>",
    ("roll", 1, True, 0): "k_pathtrace_roll<1,4,true,0>", ("roll", 1, True, 1): "k_pathtrace_roll<1,4,true,1>",
    ("roll", 2, False, 0): "k_pathtrace_roll<2,4,false,0>", ("roll", 2, False, 1): "k_pathtrace_roll<2,4,false,1>",
    ("roll", 2, True, 0): "k_pathtrace_roll<2,4,true,0>", ("roll", 2, True, 1): "k_pathtrace_roll<2,4,true,1>",
    ("wide", 1, False, 0): "k_pathtrace_roll<1,4,false,0,wide4>", ("wide", 2, False, 0): "k_pathtrace_roll<2,4,false,0,wide4>",
    ("wave", 1, False, 0, 4): "k_pathtrace<1,4,false,0>", ("wave", 1, False, 0, 1): "k_pathtrace<1,1,false,0>",
    ("wave", 1, True, 0, 4): "k_pathtrace<1,4,true,0>", ("wave", 1, True, 0, 1): "k_pathtrace<1,1,true,0>",
    ("wave", 2, False, 0, 4): "k_pathtrace<2,4,false,0>", ("wave", 2, False, 0, 1): "k_pathtrace<2,1,false,0>",
    ("wave", 2, True, 0, 4): "k_pathtrace<2,4,true,0>", ("wave", 2, True, 0, 1): "k_pathtrace<2,1,true,0>",
    # the Halton sampler has the 128-register instantiations only: waves per SIMD = 1 launches them too
    ("wave", 1, False, 1, 4): "k_pathtrace<1,4,false,1>", ("wave", 1, False, 1, 1): "k_pathtrace<1,4,false,1>",
    ("wave", 1, True, 1, 4): "k_pathtrace<1,4,true,1>", ("wave", 1, True, 1, 1): "k_pathtrace<1,4,true,1>",
    ("wave", 2, False, 1, 4): "k_pathtrace<2,4,false,1>", ("wave", 2, False, 1, 1): "k_pathtrace<2,4,false,1>",
    ("wave", 2, True, 1, 4): "k_pathtrace<2,4,true,1>", ("wave", 2, True, 1, 1): "k_pathtrace<2,4,true,1>",
    ("wg", 1, False, 0): "k_pathtrace_wg<1,false,0>", ("wg", 1, False, 1): "k_pathtrace_wg<1,false,1>",
    ("wg", 1, True, 0): "k_pathtrace_wg<1,true,0>", ("wg", 1, True, 1): "k_pathtrace_wg<1,true,1>",
    ("wg", 2, False, 0): "k_pathtrace_wg<2,false,0>", ("wg", 2, False, 1): "k_pathtrace_wg<2,false,1>",
    ("wg", 2, True, 0): "k_pathtrace_wg<2,true,0>", ("wg", 2, True, 1): "k_pathtrace_wg<2,true,1>",
}


def test_every_option_set_launches_the_instantiation_it_names(pkg, ctx, manifest, golden_blob):
    """The kernel tables of cray_hip.hip: counter level x rare features (a scene without node programs, one with; CRH_FORCE_PROGRAMS makes every scene one with) x
    sampler, the 4-ary walk, and — where the library holds them — the one-unit-at-a-time form at both register budgets and the workgroup form. Every dispatch (a
    16 x 8 region, one pass, two bounces) reports exactly the name above, and neither the counter level nor the form changes a frame: each equals the first frame
    of its scene and sampler bit for bit."""
    import os
    abi = pkg.abi
    forced = "CRH_FORCE_PROGRAMS" in os.environ
    forms = kernel_forms(pkg, ctx)
    first = {}
    try:
        for name, wide in (("cfg1_scene", False), ("nodezoo", False), ("cfg1_scene", True)):
            m = manifest[name]
            w, h = m["width"], m["height"]
            region = (w // 2 - 8, h // 2 - 4, w // 2 + 8, h // 2 + 4)
            rare = name == "nodezoo" or forced
            ctx.set_option(abi.OPT_WALK, abi.WALK_WIDE4 if wide else abi.WALK_BINARY)          # (what the next upload prepares)
            ctx.upload(pkg.api.Scene(golden_blob(m.get("blob") or name)))
            fb = ctx.framebuffer(w, h)
            cases = [(abi.KERNEL_ROLL, 4, ("wide" if wide and not rare else "roll", level, rare, samp)) for level in (1, 2) for samp in ((0,) if wide else (0, 1))]
            if not wide and abi.KERNEL_WAVE in forms:
                cases += [(abi.KERNEL_WAVE, wps, ("wave", level, rare, samp, wps)) for level in (1, 2) for samp in (0, 1) for wps in (4, 1)]
            if not wide and abi.KERNEL_WG in forms:
                cases += [(abi.KERNEL_WG, 4, ("wg", level, rare, samp)) for level in (1, 2) for samp in (0, 1)]
            for kernel, wps, key in cases:
                level, samp = key[1], key[3]
                ctx.set_option(abi.OPT_KERNEL, kernel)
                ctx.set_option(abi.OPT_WAVES_PER_SIMD, wps)
                ctx.set_option(abi.OPT_COUNTER_LEVEL, level)
                ctx.set_option(abi.OPT_SAMPLER, abi.SAMPLER_HALTON if samp else abi.SAMPLER_RANDOM)
                ctx.clear(fb, w, h)
                ctx.render_region(fb, w, h, 1, 2, region=region)
                img = ctx.download(fb, w, h)
                assert ctx.last_kernel_name() == KERNEL_NAMES[key], (name, key, ctx.last_kernel_name())
                ref = first.setdefault((name, samp), img)
                assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (name, key)
            x0, y0, x1, y1 = region
            assert first[(name, 0)][h - y1:h - y0, x0:x1].any() and not first[(name, 0)][:h - y1].any(), name          # (the region was rendered, and nothing else)
    finally:
        ctx.set_option(abi.OPT_WALK, abi.WALK_BINARY)
        ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_ROLL)
        ctx.set_option(abi.OPT_WAVES_PER_SIMD, 4)
        ctx.set_option(abi.OPT_COUNTER_LEVEL, 2)
        ctx.set_option(abi.OPT_SAMPLER, abi.SAMPLER_RANDOM)


@pytest.mark.parametrize("name", ["cfg2_hdr_small", "cfg4_statues_small"])
def test_wide_walk_meets_the_tolerance_gates(name, pkg, manifest, golden_ref):
    """The 4-ary walk at north_star's own bar on two BASELINE configs: the binary walk is the bit-exact contract and the default; WIDE4 reaches
    leaves in another order, so two candidates one rounding error apart may resolve differently (poly.c:36: strict t < distance) and a handful of paths diverge. Against the
    REFERENCE's frame (c-ray-ref-strict fixture) it must stay inside SURVEY 8(c)'s gates for a 4-spp frame — at most 0.5 % of the pixels more than 1 LSB (8-bit sRGB) away,
    RMSE at most 5e-3 — with the ray count equal up to the divergent paths."""
    api, abi = pkg.api, pkg.abi
    m = manifest[name]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    c = api.Context(0)
    try:
        c.set_option(abi.OPT_WALK, abi.WALK_WIDE4)
        c.upload(resize_camera(api.Scene(built_blob(m["built_blob"])), w, h))
        fb = c.framebuffer(w, h)
        c.reset_counters()
        c.render_region(fb, w, h, s, b)
        img, cnt = c.download(fb, w, h), c.counters()
        assert "wide4" in c.last_kernel_name(), c.last_kernel_name()
    finally:
        c.close()
    ref = golden_ref(name)

    def srgb(x):          # color.h:51-57 + the clamp of texture.c:18-22, in [0, 1]
        x = np.clip(x.astype(np.float64), 0.0, None)
        return np.clip(np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055), 0.0, 1.0)
    a, r = srgb(img), srgb(ref)
    lsb = np.abs(np.floor(a * 255.0) - np.floor(r * 255.0)).max(axis=2)
    frac = float((lsb > 1).mean())
    rmse = float(np.sqrt(((a - r) ** 2).mean()))
    differ = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
    assert frac <= 0.005 and rmse <= 5e-3, (name, frac, rmse, differ)
    assert differ <= 0.005 * w * h, (name, differ)          # (what was counted: a handful of pixels, one path each — DESIGN.md section 7)
    assert abs(cnt["rays"] - m["rays"]) <= 1e-3 * m["rays"], (cnt["rays"], m["rays"])
    assert cnt["paths"] == w * h * s


def test_error_paths(pkg, ctx, golden_blob):
    api, abi = pkg.api, pkg.abi
    fresh = api.Context(0)
    fb = fresh.framebuffer(8, 8)
    with pytest.raises(api.CrhError) as e:
        fresh.render_region(fb, 8, 8, 1, 1)             # no scene uploaded
    assert e.value.code == abi.ERR_INVALID
    fresh.upload(api.Scene(golden_blob("fence")))
    with pytest.raises(api.CrhError):
        fresh.render_region(fb, 8, 8, 1, 1, region=(0, 0, 9, 8))     # tile outside the image
    with pytest.raises(api.CrhError):
        fresh.render_region(fb, 8, 8, 2, 1, first_pass=1, pass_count=2)   # passes beyond max_passes
    fresh.render_region(fb, 8, 8, 2, 1, region=(3, 3, 3, 3))        # empty region is a no-op
    fresh.render_region(fb, 8, 8, 2, 0)                             # zero bounces: black frame
    assert not fresh.download(fb, 8, 8).any()
    with pytest.raises(api.CrhError):
        fresh.set_option(999, 1)
    fresh.close()


def test_edge_cases_empty_ragged_single_pixel(pkg, ctx, oracle, manifest, golden_blob):
    """Empty tile list, 1x1 regions, a ragged 3-tile cover, and a scene whose TLAS is empty (every ray leaves the scene)."""
    api = pkg.api
    m = manifest["glowmetal"]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    full, cnt_full, fb = gpu_render(pkg, ctx, golden_blob("glowmetal"), w, h, s, b)
    # nothing to do
    ctx.render_tiles(fb, w, h, s, b, [])
    assert np.array_equal(ctx.download(fb, w, h), full)
    # single pixels (first, last, middle) and single rows / columns reproduce the full frame's values
    ctx.clear(fb, w, h)
    regions = [(0, 0, 1, 1), (w - 1, h - 1, w, h), (w // 2, h // 2, w // 2 + 1, h // 2 + 1), (0, 3, w, 4), (5, 0, 6, h)]
    for r in regions:
        ctx.render_region(fb, w, h, s, b, region=r)
    img = ctx.download(fb, w, h)
    mask = np.zeros((h, w), bool)
    for x0, y0, x1, y1 in regions:
        mask[h - y1:h - y0, x0:x1] = True          # framebuffer rows are stored top-down (texture.c:24-28)
    assert np.array_equal(img[mask], full[mask]) and not img[~mask].any()
    # ragged cover: three tiles of unequal shape, one of them a single column
    ctx.clear(fb, w, h)
    ctx.reset_counters()
    ctx.render_tiles(fb, w, h, s, b, [(0, 0, w - 1, h // 3), (0, h // 3, w - 1, h), (w - 1, 0, w, h)])
    assert np.array_equal(ctx.download(fb, w, h), full)
    assert ctx.counters() == cnt_full
    # a world without instances: the TLAS has no nodes (bvh.c:362-365), every path is one ray into the background
    scene = api.Scene(golden_blob("glowmetal"))
    oscene = oracle.OracleScene(golden_blob("glowmetal"))
    for d in (scene.desc, oscene.desc):
        d.instance_count = 0; d.tlas_node_count = 0; d.tlas_prim_count = 0
    ctx.upload(scene)
    ctx.clear(fb, w, h)
    ctx.reset_counters()
    ctx.render_region(fb, w, h, s, b)
    img, cnt = ctx.download(fb, w, h), ctx.counters()
    ref, ocnt = oracle.render(oscene, w, h, s, b)
    assert cnt["rays"] == cnt["paths"] == ocnt["rays"] == w * h * s and cnt["node_tests"] == 0
    assert np.array_equal(img, ref)


def test_interactive_mode_halton_sampler(pkg, ctx, manifest, golden_blob, golden_ref):
    """CRH_OPT_SAMPLER = HALTON renders renderThreadInteractive's passes; progressive dispatches
    (one pass at a time, as a preview loop would) give the same frame bit for bit as one dispatch."""
    abi = pkg.abi
    m = manifest["cfg1_scene_iterative"]
    w, h, n, b = m["width"], m["height"], m["samples"], m["bounces"]
    ctx.upload(pkg.api.Scene(golden_blob(m["blob"])))
    fb = ctx.framebuffer(w, h)
    ctx.set_option(abi.OPT_SAMPLER, abi.SAMPLER_HALTON)
    try:
        ctx.reset_counters()
        ctx.render_region(fb, w, h, n, b, pass_count=m["passes"])
        img, cnt = ctx.download(fb, w, h), ctx.counters()
        ctx.clear(fb, w, h)
        for p in range(m["passes"]):
            ctx.render_region(fb, w, h, n, b, first_pass=p, pass_count=1)
        assert np.array_equal(ctx.download(fb, w, h), img)
    finally:
        ctx.set_option(abi.OPT_SAMPLER, abi.SAMPLER_RANDOM)
    assert np.array_equal(img, golden_ref("cfg1_scene_iterative"))
    assert cnt["paths"] == w * h * m["passes"]
    with pytest.raises(pkg.api.CrhError):
        ctx.set_option(abi.OPT_SAMPLER, 7)


def test_full_size_properties_cfg2(pkg, ctx, oracle):
    """BASELINE.json configs[1] at full resolution (needs scenes/_built/cfg2_hdr.blob, made by build()):
    deterministic, tile decomposition exact, ray count and every float of the frame equal to the oracle's —
    checked at 16 spp so that the CPU side stays in seconds; the 256-spp frame is what bench.py times."""
    import os
    from __graft_entry__ import BUILT
    blob = os.path.join(BUILT, "cfg2_hdr.blob")
    if not os.path.exists(blob):
        pytest.skip("scenes/_built/cfg2_hdr.blob not built")
    w, h, s, b = 1280, 720, 16, 8
    img, cnt, fb = gpu_render(pkg, ctx, blob, w, h, s, b)
    again, cnt2, _ = gpu_render(pkg, ctx, blob, w, h, s, b)
    assert np.array_equal(img, again) and cnt == cnt2
    tiles = pkg.tiles.quantize_image(w, h, 64, 64, pkg.tiles.ORDER_FROM_MIDDLE)
    ctx.clear(fb, w, h)
    for r in range(8):
        ctx.render_tiles(fb, w, h, s, b, pkg.tiles.tiles_for_rank(tiles, r, 8))
    assert np.array_equal(ctx.download(fb, w, h), img)
    oscene = oracle.OracleScene(blob)
    ref, ocnt = oracle.render(oscene, w, h, s, b)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), image_stats(img, ref)
    assert cnt["rays"] == ocnt["rays"]


def test_dropin_binary_renders_through_the_reference_program(pkg, ctx, manifest, golden_blob, golden_ref, tmp_path):
    """c-ray-hip = the reference's own main.c / loader / encoders with renderer.c replaced by renderer_hip.c.
    Its float buffer must equal the library path's and the reference's bit for bit; the BMP it writes — the reference's untouched encoder fed by
    the 8-bit frame renderer_hip.c converts on the device — must equal the real reference's file byte for byte."""
    import json
    import os
    import subprocess
    import sys
    exe, overlay, built = dropin_paths()
    if not built:
        pytest.skip("c-ray-hip or the asset overlay is not built (needs the reference's sources at build time)")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import refrun
    m = manifest["cfg1_scene"]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    scene = refrun.rewrite_scene("scene.json", w, h, s, b, out_dir=str(tmp_path))
    dump = str(tmp_path / "hip.f32")
    env = dict(os.environ, CRH_DUMP_F32=dump, CRAY_HIP_DEVICES="1", **dropin_env())
    proc = subprocess.run([exe], input=json.dumps(scene).encode(), cwd=overlay, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, timeout=600)
    assert proc.returncode == 0, proc.stdout.decode(errors="replace")[-2000:]
    img = np.fromfile(dump, dtype=np.float32).reshape(h, w, 3)
    lib_img, _, _ = gpu_render(pkg, ctx, golden_blob("cfg1_scene"), w, h, s, b)
    assert np.array_equal(img, lib_img)
    assert np.array_equal(img, golden_ref("cfg1_scene"))
    bmp = [f for f in os.listdir(tmp_path) if f.endswith(".bmp")]
    assert bmp, "the reference's encoder wrote no image"
    import hashlib
    data = open(tmp_path / bmp[0], "rb").read()
    assert data[:2] == b"BM" and len(data) >= w * h * 3
    # byte for byte the file the real reference writes (tools/gen_bmp_golden.py): its encoder, fed by an 8-bit frame that was converted on the device
    assert hashlib.md5(data).hexdigest() == m["bmp_md5"], "the BMP differs from c-ray-ref-strict's"
    os.remove(tmp_path / bmp[0])
    # where renderFrame()'s time went (CRH_DUMP_STATS): frame_ms runs to the END of renderFrame() — set-up + render phase + teardown — with the contexts made from
    # newRenderer() on (the default) and with every context made inside the frame (CRH_DROPIN_NO_PREFETCH); the same frame either way
    for extra in ({}, {"CRH_DROPIN_NO_PREFETCH": "1"}):
        stats = str(tmp_path / "stats.json")
        proc = subprocess.run([exe], input=json.dumps(scene).encode(), cwd=overlay, env=dict(env, CRH_DUMP_STATS=stats, **extra), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, timeout=600)
        assert proc.returncode == 0, proc.stdout.decode(errors="replace")[-2000:]
        st = json.load(open(stats))
        assert st["rays"] == m["rays"] and st["gpus"] == 1
        assert st["teardown_ms"] >= 0 and st["setup_ms"] > 0 and st["render_phase_ms"] > 0
        assert abs(st["frame_ms"] - (st["setup_ms"] + st["render_phase_ms"] + st["teardown_ms"])) < 0.01, st
        assert st["setup_ms"] >= st["upload_ms"] and st["setup_ms"] >= st["flatten_ms"], st
        assert np.array_equal(np.fromfile(dump, dtype=np.float32).reshape(h, w, 3), img)
        for f in os.listdir(tmp_path):
            if f.endswith(".bmp"): os.remove(tmp_path / f)
    # --iterative: the interactive mode of the same program (Halton sampler, passes 1 .. samples-1, progressive chunks)
    mi = manifest["cfg1_scene_iterative"]
    scene = refrun.rewrite_scene("scene.json", w, h, mi["samples"], mi["bounces"], out_dir=str(tmp_path))
    proc = subprocess.run([exe, "--iterative"], input=json.dumps(scene).encode(), cwd=overlay, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, timeout=600)
    assert proc.returncode == 0, proc.stdout.decode(errors="replace")[-2000:]
    img = np.fromfile(dump, dtype=np.float32).reshape(h, w, 3)
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    fb = ctx.framebuffer(w, h)
    ctx.set_option(pkg.abi.OPT_SAMPLER, pkg.abi.SAMPLER_HALTON)
    try:
        ctx.render_region(fb, w, h, mi["samples"], mi["bounces"], pass_count=mi["passes"])
        assert np.array_equal(img, ctx.download(fb, w, h))
    finally:
        ctx.set_option(pkg.abi.OPT_SAMPLER, pkg.abi.SAMPLER_RANDOM)
    assert np.array_equal(img, golden_ref("cfg1_scene_iterative"))
    bmp = [f for f in os.listdir(tmp_path) if f.endswith(".bmp")]
    assert bmp and hashlib.md5(open(tmp_path / bmp[0], "rb").read()).hexdigest() == mi["bmp_md5"], "the --iterative BMP differs from c-ray-ref-strict's"


def test_c_host_reduce_goes_through_rccl(pkg, manifest, golden_blob, tmp_path):
    """crh_frames_reduce (the C host's frame assembly) on the one GPU that is here: with CRH_FORCE_RCCL the single-rank case
    takes the real path (dlopen librccl, ncclCommInitAll, grouped in-place ncclReduce on the context's stream) and must
    leave the frame unchanged. Runs in its own process (the RCCL communicator is process-wide state)."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = manifest["fence"]
    code = f"""
import sys, numpy as np
sys.path.insert(0, {repo!r})
from __graft_entry__ import load_package
pkg = load_package(); api = pkg.api
ctx = api.Context(0); ctx.upload(api.Scene({golden_blob("fence")!r}))
w, h, s, b = {m["width"]}, {m["height"]}, {m["samples"]}, {m["bounces"]}
fb = ctx.framebuffer(w, h); ctx.render_region(fb, w, h, s, b)
before = ctx.download(fb, w, h)
ctx.frames_reduce(fb, w, h); ctx.frames_reduce(fb, w, h)
after = ctx.download(fb, w, h)
assert before.any() and np.array_equal(before, after)
print("reduce ok")
"""
    proc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CRH_FORCE_RCCL="1"), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, timeout=600)
    assert proc.returncode == 0 and b"reduce ok" in proc.stdout, proc.stdout.decode(errors="replace")[-2000:]


def test_bench_reduce_path_with_a_one_rank_rccl_group(pkg, manifest, golden_blob):
    """bench.py's N > 1 step (FrameRenderer.render + torch.distributed.reduce over backend nccl = RCCL) with the one rank
    that can exist here: process group on 127.0.0.1, the framebuffer tensor reduced in place on the renderer's stream."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = manifest["fence"]
    code = f"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r})
from __graft_entry__ import load_package
pkg = load_package()
dist.init_process_group(backend="nccl", rank=0, world_size=1)
w, h, s, b = {m["width"]}, {m["height"]}, {m["samples"]}, {m["bounces"]}
fr = pkg.render.FrameRenderer(pkg.api, pkg.api.Scene({golden_blob("fence")!r}), w, h, device=0, rank=0, world=1, tile=(32, 32))
fr.render(s, b); torch.cuda.synchronize(); before = fr.fb.cpu().numpy().copy()
for _ in range(2):
    fr.render(s, b)
    with torch.cuda.stream(fr.stream):
        dist.reduce(fr.fb, dst=0, op=dist.ReduceOp.SUM)
dist.barrier(); torch.cuda.synchronize()
assert before.any() and np.array_equal(fr.fb.cpu().numpy(), before)
dist.destroy_process_group()
print("nccl reduce ok")
"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", HSA_ENABLE_IPC_MODE_LEGACY="0")
    proc = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert proc.returncode == 0 and b"nccl reduce ok" in proc.stdout, proc.stdout.decode(errors="replace")[-2000:]


def test_frame_renderer_on_torch_stream(pkg, ctx, manifest, golden_blob):
    """The torch.distributed host (render.py): kernels on a torch stream, framebuffer = torch tensor. Same frame as the
    plain C-ABI path, for the full tile list and for an interleaved 1-of-2 share (the other half stays exactly zero)."""
    import torch
    m = manifest["refraction"]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    full, _, _ = gpu_render(pkg, ctx, golden_blob("refraction"), w, h, s, b)
    scene = pkg.api.Scene(golden_blob("refraction"))
    fr = pkg.render.FrameRenderer(pkg.api, scene, w, h, device=0, rank=0, world=1, tile=(32, 32))
    fr.render(s, b)
    fr.reduce(None)
    torch.cuda.synchronize()
    assert np.array_equal(fr.fb.cpu().numpy(), full)
    fr.render(s, b)                       # re-rendering clears first: same frame again
    torch.cuda.synchronize()
    assert np.array_equal(fr.fb.cpu().numpy(), full)
    fr.close()
    parts = []
    for r in range(2):
        f2 = pkg.render.FrameRenderer(pkg.api, scene, w, h, device=0, rank=r, world=2, tile=(32, 32))
        f2.render(s, b)
        torch.cuda.synchronize()
        parts.append(f2.fb.cpu().numpy())
        f2.close()
    assert np.array_equal(parts[0] + parts[1], full)
    assert not (np.abs(parts[0]) * np.abs(parts[1])).any()      # disjoint ownership


@pytest.mark.parametrize("float_tiles", [False, True], ids=["srgb8", "float"])
def test_cluster_worker_renders_its_tiles_on_the_gpu(float_tiles, pkg, oracle, manifest, golden_ref):
    """`c-ray-hip --worker` is the reference's network worker (handshake, asset / scene transfer, tile protocol:
    src/utils/protocol/worker.c compiled unmodified) with its render threads replaced by one GPU dispatch thread. A minimal master in
    this test speaks the reference's wire protocol (networking.c:44-131 framing, server.c:45-52, 296-345, 148-175 messages): it syncs
    input/scene.json, hands out 32x32 tiles, and every 8-bit sRGB tile the worker submits must equal, byte for byte, that tile of the
    real reference's frame (golden fixture through colorToSRGB, renderer.c:294-300 = worker.c:176-181).
    (The reference's own master is not used: in v0.6.3 it pastes tiles with a row slip (server.c:166), dies of SIGPIPE when the worker
    closes first, and corrupts its heap with -j 0; it is marked experimental upstream.)
    float: CRH_WORKER_FLOAT_TILES=1 — the same tiles as linear float means (protocol.c:102-127 carries isFloatPrecision): equal to the reference's
    float buffer bit for bit."""
    import base64
    import json
    import os
    import socket
    import struct
    import subprocess
    import sys
    import time
    gpu_worker, overlay, built = dropin_paths()
    if not built:
        pytest.skip("c-ray-hip / the asset overlay are not built (needs the reference's sources at build time)")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import refrun
    m = manifest["cfg1_scene"]
    w, h = m["width"], m["height"]
    expected8 = oracle.to_srgb8(golden_ref("cfg1_scene"))                      # stored rows run top-down (texture.c:24-28)

    CHUNK = 1024
    def send(sock, obj):
        data = json.dumps(obj).encode() + b"\0"
        padded = data.ljust((len(data) + CHUNK - 1) // CHUNK * CHUNK, b"\0")
        sock.sendall(struct.pack(">Q", len(data)) + padded)
    def recv_exact(sock, n):
        buf = b""
        while len(buf) < n:
            part = sock.recv(n - len(buf))
            if not part:
                return None
            buf += part
        return buf
    def recv(sock):
        head = recv_exact(sock, 8)
        if not head:
            return None
        n, = struct.unpack(">Q", head)
        if n == 0:
            return None
        body = recv_exact(sock, (n + CHUNK - 1) // CHUNK * CHUNK)
        return json.loads(body[:n].rstrip(b"\0").decode())

    files = []
    for sub in ("", "shapes", "HDRs"):
        d = os.path.join(overlay, sub)
        for f in sorted(os.listdir(d)):
            path = os.path.join(d, f)
            if os.path.isfile(path) and os.path.getsize(path) < 4 << 20 and not f.endswith(".json"):
                data = base64.b64encode(open(path, "rb").read()).decode()
                rel = os.path.join(sub, f) if sub else f
                files += [{"path": "./" + rel, "data": data}, {"path": rel, "data": data}]
    scene = refrun.rewrite_scene("scene.json", w, h, m["samples"], m["bounces"], tile=(32, 32), out_dir="/tmp")
    tiles = pkg.tiles.quantize_image(w, h, 32, 32, pkg.tiles.ORDER_FROM_MIDDLE)

    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    extra = {"CRH_WORKER_FLOAT_TILES": "1"} if float_tiles else {}
    worker = subprocess.Popen([gpu_worker, "--worker", str(port)], cwd=overlay, env=dict(os.environ, CRAY_HIP_DEVICES="1", **extra, **dropin_env()),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    got = {}
    try:
        sock = None
        for _ in range(100):                       # wait for the worker to listen
            try:
                sock = socket.create_connection(("127.0.0.1", port), timeout=0.5)
                break
            except OSError:
                time.sleep(0.1)
        assert sock is not None, "the worker never listened"
        sock.settimeout(120)
        send(sock, {"action": "handshake", "version": "0.1", "githash": "NoHash"})
        assert recv(sock) == {"action": "startSync"}
        send(sock, {"action": "loadAssets", "files": files})
        assert recv(sock) == {"action": "ok"}
        send(sock, {"action": "loadScene", "data": scene, "assetPath": "./"})
        ready = recv(sock)
        assert ready and ready.get("action") == "ready" and ready.get("threadCount", 0) >= 1, ready
        send(sock, {"action": "startRender"})
        nxt = 0
        while True:
            req = recv(sock)
            assert req is not None, "the worker hung up before saying goodbye"
            act = req.get("action")
            if act == "getWork":
                if nxt < len(tiles):
                    x0, y0, x1, y1 = tiles[nxt]
                    send(sock, {"action": "newWork", "tile": {"width": x1 - x0, "height": y1 - y0, "beginX": x0, "beginY": y0, "endX": x1, "endY": y1, "tileNum": nxt}})
                    nxt += 1
                else:
                    send(sock, {"action": "renderComplete"})
            elif act == "submitWork":
                t, r = req["tile"], req["result"]
                assert bool(r["isFloatPrecision"]) == float_tiles and r["channels"] == 3 and r["width"] == t["width"] and r["height"] == t["height"]
                got[t["tileNum"]] = (t, np.frombuffer(base64.b64decode(r["data"]), np.float32 if float_tiles else np.uint8).reshape(r["height"], r["width"], 3))
                send(sock, {"action": "ok"})
            elif act == "stats":
                pass
            elif act == "goodbye":
                break
            else:
                pytest.fail(f"unexpected message from the worker: {req}")
        sock.close()
    finally:
        worker.kill()
        wlog = worker.communicate()[0].decode(errors="replace")
    assert sorted(got) == list(range(len(tiles))), (sorted(got), wlog[-1500:])
    for num, (t, px) in got.items():
        x0, y0, x1, y1 = tiles[num]
        assert (t["beginX"], t["beginY"], t["endX"], t["endY"]) == (x0, y0, x1, y1)
        want = golden_ref("cfg1_scene")[h - y1:h - y0, x0:x1] if float_tiles else expected8[h - y1:h - y0, x0:x1]
        assert np.array_equal(px.view(np.uint32) if float_tiles else px, want.view(np.uint32) if float_tiles else want), f"tile {num} {tiles[num]} differs from the reference's frame"


PROBE_VARIANTS = [(4, 12, True, 1), (4, 12, True, 0), (4, 12, True, 3), (5, 12, True, 3), (6, 7, True, 3), (7, 3, True, 3), (8, 4, False, 3)]          # (waves per SIMD, LDS stack entries, instance records in LDS, form of the node run)


@pytest.mark.parametrize("name", ["cfg1_scene", "fence"])
def test_walk_probe_equals_the_plain_walk_on_the_path_tracers_own_rays(name, pkg, ctx, manifest, golden_blob):
    """Round 6's measurement kernel (csrc/walk_probe.h: the render kernel's walk on its own, at 4 - 8 waves per SIMD) is held to the walk's bar: the counting kernel
    records every ray its waves start (crh_debug_ray_dump; as many as the dispatch counts), k_walk_probe walks them in every variant the measurement uses, and every hit
    — distance, barycentrics, BLAS prim slot, instance, bit patterns — equals the one-ray-per-lane walk's (k_trace_rays' loop); a stretch of them also goes through crh_trace_rays."""
    m = manifest[name]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    ctx.set_option(pkg.abi.OPT_COUNTER_LEVEL, 2)
    ctx.upload(pkg.api.Scene(golden_blob(name)))
    fb = ctx.framebuffer(w, h)
    try:
        cap = 1 << 11
        while True:          # (a wave's region must hold every ray the wave starts: 4096 waves on the MI355X, a few dozen on the kernel emulation)
            ctx.ray_dump(cap)
            ctx.clear(fb, w, h)
            ctx.reset_counters()
            ctx.render_region(fb, w, h, s, b)
            cnt = ctx.counters()
            total, per = ctx.ray_dump_counts()
            if per.max() < cap or cap >= 1 << 19:
                break
            cap *= 4
        assert total == cnt["rays"] == m["rays"], (total, cnt["rays"], m["rays"])          # every ray of the frame was recorded (no wave overran its region)
        ms, rays = ctx.walk_probe(0, slot=0)
        assert rays == total
        for wps, nlds, inst, fused in PROBE_VARIANTS:
            ms, rays = ctx.walk_probe(wps, nlds, inst, fused, unit_rays=128, slot=1)
            assert rays == total
            assert ctx.walk_probe_compare() == 0, (wps, nlds, inst, fused, ctx.last_kernel_name())
        wave = int(np.argmax(per))
        n = int(min(per[wave], 4096))
        r6 = ctx.ray_dump_fetch(wave, 0, n)
        hits, inst = ctx.walk_probe_fetch(1, wave, 0, n)
        ref = ctx.trace_rays(r6)
        assert np.array_equal((inst >= 0), (ref["inst"] >= 0))
        hit = inst >= 0
        assert hit.sum() > 50
        assert np.array_equal(hits[hit, 0].view(np.uint32), ref["distance"][hit].view(np.uint32))
    finally:
        ctx.ray_dump(0)
        ctx.set_option(pkg.abi.OPT_WAVE_STATS, 0)
