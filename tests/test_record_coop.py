"""The rolling kernel's quad-cooperative path-record access (c-ray_amd/csrc/cray_hip.hip: PathTab::loadRec4 / storeRec4) moves the same words.

In the lean instantiations of k_pathtrace_roll (no node programs, no volumes) the SHADE, GEN and MISS steps read and write a path's 64-B record four
lanes at a time — a quad fetches or stores one aligned 64-B line per instruction and a 4 x 4 exchange inside the quad (DPP quad permutes) hands every
lane its own record — and a walk that ended in a miss no longer leaves a hit part (CRH_REC_COOP_LOAD, CRH_REC_COOP_STORE, CRH_MISS_SKIP_HIT).

CPU tier: the kernel emulation (tests/emu) is built a second time with all three switches at 0 — the parent's record access — and a third time with all
three at 1 (the cooperative read is off by default: it did not pay on the GPU, but it stays correct), and the three libraries render the same fixtures:
frames, the counters of counter level 2 and the lanes the scheduler's steps served must be identical, and each frame must equal the reference's float
buffer bit for bit. nodezoo and volumes run the rare-features instantiations, which keep the plain access in every build.

GPU tier (-m gpu): the smallest shapes at which the exchange can go wrong, against the oracle on the same blob, bit for bit and with equal ray counts: a
single path slot in use (one partial quad, lanes 1..63 idle), batches whose size is no multiple of four with continuing and ending paths mixed inside a
quad, tiles one, two and three pixels wide, and a scene with emission (non-zero radiance words through the exchange).

The variant builds and the child that renders the fixtures are tests/emu_variants.py's.
"""
import numpy as np
import pytest

from emu_variants import build_variants, render_with_each
from support import ctx  # noqa: F401 (the module-scoped device context)

SWITCHES = ("CRH_REC_COOP_LOAD", "CRH_REC_COOP_STORE", "CRH_MISS_SKIP_HIT")


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(the emulation library as built, the same source with the three switches at 0, ... and at 1)"""
    return build_variants(tmp_path_factory.mktemp("coop"), {f"coop{v}": [f"-D{s}={v}" for s in SWITCHES] for v in (0, 1)})


def test_cooperative_record_access_is_bit_identical_to_the_plain_access(libs):
    coop, plain, all_on = render_with_each(libs)
    for a, b, c in zip(coop, plain, all_on):
        assert a["kernel"].startswith("k_pathtrace_roll<2,4,"), a
        assert a == b and a == c, (a, b, c)          # frame md5, level-2 counters, u_node / u_shade / u_swap lane sums
        assert a["ref_equal"] in (True, None), a
        assert a["counters"]["rays"] > 0
    assert any(",false," in r["kernel"] for r in coop) and any(",true," in r["kernel"] for r in coop), [r["kernel"] for r in coop]


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------
def against_oracle(pkg, ctx, oracle, blob, w, h, spp, bounces, tiles, lean=True):
    """Render the tiles on the GPU (one dispatch) and with the oracle; the frames must be equal bit for bit, the ray counts equal, nothing outside the tiles touched.
    lean: the scene must have run a lean instantiation — the one with the cooperative access."""
    ctx.upload(pkg.api.Scene(blob))
    fb = ctx.framebuffer(w, h)
    ctx.reset_counters()
    if len(tiles) == 1:
        ctx.render_region(fb, w, h, spp, bounces, region=tiles[0])
    else:
        ctx.render_tiles(fb, w, h, spp, bounces, tiles)
    img, cnt = ctx.download(fb, w, h), ctx.counters()
    assert (",false," in ctx.last_kernel_name()) == lean, ctx.last_kernel_name()
    oscene = oracle.OracleScene(blob)
    ref = np.zeros((h, w, 3), np.float32)
    rays = 0
    inside = np.zeros((h, w), bool)
    for t in tiles:
        _, ocnt = oracle.render(oscene, w, h, spp, bounces, region=t, fb=ref, threads=2)
        rays += ocnt["rays"]
        inside[h - t[3]:h - t[1], t[0]:t[2]] = True
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), int((img.view(np.uint32) != ref.view(np.uint32)).sum())
    assert cnt["rays"] == rays and cnt["paths"] == int(inside.sum()) * spp, (cnt, rays)
    assert not img[~inside].any()
    return img


@pytest.mark.gpu
def test_one_pixel_region_one_partial_quad(pkg, ctx, oracle, manifest, golden_blob):
    """1 x 1 pixel at 3 spp: every batch holds at most three paths — one quad, partly filled — and 61 lanes only lend their slot-0 address."""
    m = manifest["refraction"]
    w, h = m["width"], m["height"]
    against_oracle(pkg, ctx, oracle, golden_blob("refraction"), w, h, 3, 8, [(w // 2, h // 2, w // 2 + 1, h // 2 + 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["refraction", "cfg1_scene"])
def test_odd_region_mixes_continuing_and_ending_paths_inside_quads(name, pkg, ctx, oracle, manifest, golden_blob):
    """13 x 7 pixels at 5 spp, 8 bounces: 455 paths — batches of n not a multiple of 4; hits, misses and ended paths share quads."""
    m = manifest[name]
    w, h = m["width"], m["height"]
    x0, y0 = w // 2 - 6, h // 2 - 3
    img = against_oracle(pkg, ctx, oracle, golden_blob(name), w, h, 5, 8, [(x0, y0, x0 + 13, y0 + 7)])
    assert img.any()


@pytest.mark.gpu
def test_tiles_one_two_and_three_pixels_wide(pkg, ctx, oracle, manifest, golden_blob):
    m = manifest["refraction"]
    w, h = m["width"], m["height"]
    x, y = w // 2 - 10, h // 2 - 4
    against_oracle(pkg, ctx, oracle, golden_blob("refraction"), w, h, 5, 8, [(x, y, x + 1, y + 9), (x + 5, y, x + 7, y + 9), (x + 11, y + 1, x + 14, y + 8)])


@pytest.mark.gpu
def test_emission_goes_through_the_exchange(pkg, ctx, oracle, manifest, golden_blob):
    """64 x 64 pixels at 4 spp on glowmetal: emitters, so the radiance words of continuing paths are non-zero when SHADE writes and re-reads them. (Its materials
    are node programs: the fixture runs the rare-features instantiation, whose record access is the plain one — it guards the `!PROG` condition of the switches;
    in the lean cases above the radiance words are non-zero from the first environment or emitter hit on as well.)"""
    m = manifest["glowmetal"]
    w, h = m["width"], m["height"]
    x0, y0 = (w - 64) // 2, (h - 64) // 2
    img = against_oracle(pkg, ctx, oracle, golden_blob("glowmetal"), w, h, 4, m["bounces"], [(x0, y0, x0 + 64, y0 + 64)], lean=False)
    assert img.any()
