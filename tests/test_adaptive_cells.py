"""Adaptive sampling at cell granularity within each rectangle (crh_adaptive_step_cells, crh_render_adaptive_cells; k_adaptive_cells in c-ray_amd/csrc/adaptive.h):
the rectangle stays the unit of work and of the interface, the decision is made per cell of c x c pixels inside it, optionally widened by one cell (dilation never
crosses a rectangle's edge).

The step's arithmetic is part of the interface (include/cray_hip.h). `restatement_cells` below is that arithmetic in NumPy float32 — the cells' anchoring and order,
the 64 strided partial sums, the tree over them, the decision from the neighbours' flags — and the GPU tier holds the kernel to it bit for bit: errors, flags and the
half-sample frame afterwards. On a rendered scene every cell of an adaptive frame is, bit for bit, the uniform render at the pass count the cell stopped at, its
half-sample frame the uniform render at half of that, and the whole loop is replayed in NumPy on the uniform frames alone. The CPU tier runs this file's GPU tests
on the kernel emulation (tests/emu)."""
import ctypes as C
import os

import numpy as np
import pytest

from adaptive_spec import (CAP, EMAX, H2, INF, TILE, W2, api_threshold_and_frame, frames, grid, pixel_errors, restatement, run_dropin, strip_cut_rectangles, tile_lists,
                           two_noise_levels)
from denoise_spec import restatement_v
from support import DeviceArray, assert_bit_equal, bits, ctx, dropin_env, dropin_paths, emulated_dropin, f32, header_values, run_gpu_tests_on_emulation, same_bits  # noqa: F401 (ctx: the fixture)


# ---- the restatement (include/cray_hip.h: crh_adaptive_step_cells) ----------------------------------------------------------------------------
def cell_grid(tile, c):
    x0, y0, x1, y1 = tile
    return -(-(x1 - x0) // c), -(-(y1 - y0) // c)


def cell_offsets(tiles, c):
    """offset[r] = the index of rectangle r's first cell; offset[len(tiles)] = the total."""
    out = [0]
    for t in tiles:
        cx, cy = cell_grid(t, c)
        out.append(out[-1] + cx * cy)
    return np.array(out, np.uint32)


def cell_slices(H, tile, c):
    """The cells of one rectangle in index order (j cx + i): stored rows and columns of each, anchored at the rectangle's first stored row and first column."""
    x0, y0, x1, y1 = tile
    cx, cy = cell_grid(tile, c)
    top = H - y1
    return [np.s_[top + j * c:min(top + (j + 1) * c, H - y0), x0 + i * c:min(x0 + (i + 1) * c, x1)] for j in range(cy) for i in range(cx)]


def cell_error(ek):
    """E of one cell from its pixels' errors in enumeration order: lane l adds e_k for k = l, l + 64, ... ascending, then the tree over the 64 partials."""
    n = ek.size
    P = np.zeros(64, f32)
    for first in range(0, n, 64):
        m = min(64, n - first)
        P[:m] = P[:m] + ek[first:first + m]
    stride = 32
    while stride >= 1:
        P[:stride] = P[:stride] + P[stride:2 * stride]
        stride //= 2
    E = P[0] / f32(n)
    assert E.dtype == np.float32
    return E


def cell_errors(fb, half, tiles, c):
    """E of every cell as if all were live (a cell that is not live reports 0)."""
    H = fb.shape[0]
    e = pixel_errors(fb, half)
    return np.array([cell_error(e[sl].ravel()) for t in tiles for sl in cell_slices(H, t, c)], f32)


def decide(all_errors, tiles, c, threshold, dilate, live=None):
    """errors and go flags of one step from the all-live errors."""
    total = len(all_errors)
    live = np.ones(total, bool) if live is None else np.asarray(live, bool)
    errors = np.where(live, all_errors, f32(0)).astype(f32)
    hot = live & ~(errors <= f32(threshold))
    go = hot.copy()
    if dilate:
        off = cell_offsets(tiles, c)
        for r, t in enumerate(tiles):
            cx, cy = cell_grid(t, c)
            h = hot[off[r]:off[r + 1]].reshape(cy, cx)
            padded = np.zeros((cy + 2, cx + 2), bool)
            padded[1:-1, 1:-1] = h
            near = np.zeros((cy, cx), bool)
            for dj in (0, 1, 2):
                for di in (0, 1, 2):
                    near |= padded[dj:dj + cy, di:di + cx]
            go[off[r]:off[r + 1]] = (live[off[r]:off[r + 1]].reshape(cy, cx) & near).ravel()
    return errors, go


def advance(fb, half, tiles, c, go):
    """The half-sample frame after a step: fb's raw bits over the cells that go on."""
    H = fb.shape[0]
    after = half.copy()
    k = 0
    for t in tiles:
        for sl in cell_slices(H, t, c):
            if go[k]:
                after[sl] = fb[sl]
            k += 1
    return after


def restatement_cells(fb, half, tiles, c, threshold, dilate, live=None, all_errors=None):
    """errors float32 [cells], go bool [cells], and the half-sample frame afterwards."""
    if all_errors is None:
        all_errors = cell_errors(fb, half, tiles, c)
    errors, go = decide(all_errors, tiles, c, threshold, dilate, live)
    return errors, go, advance(fb, half, tiles, c, go)


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------
def gpu_step_cells(pkg, ctx, fb, half, tiles, c, threshold, dilate, live=None):
    """Context.adaptive_step_cells on copies of fb and half: errors, flags, the half-sample frame afterwards; the frame must come back untouched."""
    h, w = fb.shape[:2]
    dfb, dhalf = DeviceArray(pkg, fb), DeviceArray(pkg, half)
    errors, flags = ctx.adaptive_step_cells(dfb.ptr, dhalf.ptr, w, h, tiles, c, threshold, dilate=dilate, live=live)
    assert np.array_equal(bits(dfb.read(ctx)), bits(fb)), "the frame was written"
    return errors, flags, dhalf.read(ctx)


# ---- 1. the step equals the restatement bit for bit --------------------------------------------------------------------------------------------
CASES = {"1x1-c1": ("1x1", 1), "3x2-c2": ("3x2", 2), "37x29-c8": ("37x29", 8), "300x5-c16": ("300x5", 16), "161x75-64x64-c8": ("161x75-64x64", 8),
         "161x75-64x64-c16": ("161x75-64x64", 16), "161x75-sparse-c8": ("161x75-sparse", 8), "161x75-corners-c8": ("161x75-corners", 8), "32x32-c1": (None, 1)}


def case(pkg, name):
    lists = tile_lists(pkg)
    key, c = CASES[name]
    w, h, tiles = (32, 32, [(0, 0, 32, 32)]) if key is None else lists[key]
    return w, h, tiles, c


def across_an_edge(w, h, tiles, c, hot, go):
    """Pairs of horizontally or vertically adjacent pixels that lie in different rectangles, one in a hot cell, the other in a cell that does not go on."""
    ident, cell = np.full((h, w), -1), np.full((h, w), -1)
    k = 0
    for r, t in enumerate(tiles):
        for sl in cell_slices(h, t, c):
            ident[sl], cell[sl] = r, k
            k += 1
    n = 0
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :])):
        for p, q in ((a, b), (b, a)):
            both = (ident[p] >= 0) & (ident[q] >= 0) & (ident[p] != ident[q])
            n += int((both & hot[cell[p]] & ~go[cell[q]]).sum())
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_cell_step_equals_the_restatement_bit_for_bit(name, pkg, ctx):
    w, h, tiles, c = case(pkg, name)
    fb, half = frames(w, h)
    for a in (fb, half):
        assert np.isnan(a).any() and np.isinf(a).any() and (a < 0).any(), "the frame and the half-sample frame hold a NaN, an inf and a negative channel each"
    if w > 2 and h > 2:
        assert pixel_errors(fb, half)[1, 1] == EMAX
    covered = np.zeros((h, w), bool)
    for x0, y0, x1, y1 in tiles:
        covered[h - y1:h - y0, x0:x1] = True
    off = cell_offsets(tiles, c)
    total = int(off[-1])
    assert np.array_equal(pkg.api.adaptive_cell_offsets(tiles, c), off)
    base = cell_errors(fb, half, tiles, c)
    assert len(base) == total and np.isfinite(base).all() and (base >= 0).all()
    if name == "32x32-c1":
        assert total == pkg.abi.ADAPTIVE_CELLS_MAX == 1024, "exactly the most cells a rectangle may hold"
    if name == "300x5-c16":
        assert all(sl[1].stop - sl[1].start == 16 and sl[0].stop - sl[0].start == 5 for sl in cell_slices(h, tiles[0], c)[:-1]), "80-pixel cells: two rounds, the second ragged"
    median = float(np.median(base))
    pick = total // 2
    exact = float(base[pick])          # one cell's own error: E <= threshold holds with equality, the cell stops (unless a neighbour keeps it)
    rng = np.random.default_rng(5)
    half_mask = rng.random(total) < 0.5
    one_rect = np.ones(total, bool)
    one_rect[off[len(tiles) // 2]:off[len(tiles) // 2 + 1]] = False          # one rectangle with no live cell (the only one, where there is one: nothing is launched)
    masks = {"all": None, "half": half_mask, "one rectangle dead": one_rect, "none": np.zeros(total, bool)}
    if name == "161x75-64x64-c8":
        assert total == 210 and len(set(base.tolist())) == 209, (total, len(set(base.tolist())))
        counts = {d: int(decide(base, tiles, c, median, d)[1].sum()) for d in (0, 1)}
        print(f"{name}: at the median {counts[0]} cells go on without dilation, {counts[1]} with")
        assert counts == {0: 105, 1: 122}, "input condition: dilation adds cells and does not add all"
        go = decide(base, tiles, c, median, 1)[1]
        assert any(0 < go[off[r]:off[r + 1]].sum() < off[r + 1] - off[r] for r in range(len(tiles))), "with dilation a rectangle holds both flag values"
        hot = ~(base <= f32(median))
        assert across_an_edge(w, h, tiles, c, hot, go) > 0, "input condition: a hot cell has a neighbour across a rectangle's edge that does not go on"
    for dilate in (0, 1):
        for what, threshold in (("0", 0.0), ("inf", INF), ("median", median), ("exact", exact)):
            for mask_name, live in masks.items():
                want_e, want_f, want_half = restatement_cells(fb, half, tiles, c, threshold, dilate, live, all_errors=base)
                got_e, got_f, got_half = gpu_step_cells(pkg, ctx, fb, half, tiles, c, threshold, dilate, live)
                tag = f"{name} dilate {dilate} threshold {what} live {mask_name}"
                print(f"{tag}: continuing {int(want_f.sum())} of {total}")
                assert_bit_equal(got_e, want_e, f"{tag}: errors")
                assert np.array_equal(got_f, want_f), (tag, np.flatnonzero(got_f != want_f))
                same_bits(got_half, want_half, f"{tag}: the half-sample frame afterwards")
                # (what the restatement's answer means, spelled out on the device's buffers)
                k = 0
                for t in tiles:
                    for sl in cell_slices(h, t, c):
                        assert np.array_equal(bits(got_half[sl]), bits(fb[sl] if got_f[k] else half[sl])), (tag, k)
                        k += 1
                assert np.array_equal(bits(got_half[~covered]), bits(half[~covered])), "a pixel in no rectangle was touched"
                if live is not None:
                    assert not got_f[~live].any() and (got_e[~live] == 0).all(), "a cell that is not live reports 0 and does not go on"
                if what == "inf" or mask_name == "none":
                    assert not got_f.any() and np.array_equal(bits(got_half), bits(half))
                if what == "0" and live is None and not dilate:
                    assert np.array_equal(got_f, base > 0)
                if what == "exact" and live is None and not dilate:
                    assert not got_f[pick], "E <= threshold with equality: the cell stops"
                    if exact > 0:          # ... and one ulp below it goes on
                        below = float(np.nextafter(f32(exact), f32(0)))
                        assert gpu_step_cells(pkg, ctx, fb, half, tiles, c, below, 0)[1][pick]
                if name == "161x75-64x64-c8" and what == "median" and live is None and dilate:
                    hot = ~(got_e <= f32(median))
                    assert across_an_edge(w, h, tiles, c, hot, got_f) > 0, "a hot cell's neighbour across a rectangle's edge is not dilated into"


# ---- 2. every cell of an adaptive frame is a uniform frame, and the loop is replayable ------------------------------------------------------------
CELL2 = 8


def replay(uniform, tiles, c, m, cap, threshold, dilate):
    """crh_render_adaptive_cells on the uniform frames alone: a live cell's frame at count n is uniform[n], its half uniform[n / 2]. (passes, errors) per cell."""
    total = int(cell_offsets(tiles, c)[-1])
    live = np.ones(total, bool)
    passes, errors = np.zeros(total, np.int32), np.zeros(total, f32)
    n = m
    while True:
        last = n == cap
        e, go, _ = restatement_cells(uniform[n], uniform[n // 2], tiles, c, INF if last else threshold, dilate, live)
        if not last and threshold == 0.0:
            go = live.copy()
        done = live & ~go
        passes[done], errors[done] = n, e[done]
        live = go
        if not live.any():
            return passes, errors
        n *= 2


@pytest.fixture(scope="module")
def rendered(pkg, ctx, manifest, golden_blob):
    """glowmetal at 160 x 100, rectangles 32 x 20, cells of 8 (4 x 3 a rectangle, the last row 4 high), min_passes 2, cap 16 of max_passes 16: the uniform frames
    at 1, 2, 4, 8 and 16 passes (once each), the errors of a measure-only step at 2 passes done by hand, and the adaptive renders at the median of the nonzero
    ones with and without dilation."""
    w, h = W2, H2
    bounces = manifest["glowmetal"]["bounces"]
    ctx.upload(pkg.api.Scene(golden_blob("glowmetal")))
    tiles = grid(pkg, w, h, 32, 20)
    assert len(tiles) == 25
    uniform = {}
    for n in (1, 2, 4, 8, 16):
        fb = ctx.framebuffer(w, h)
        ctx.render_region(fb, w, h, CAP, bounces, first_pass=0, pass_count=n)
        uniform[n] = ctx.download(fb, w, h)
        uniform[n].setflags(write=False)
    fb, half = ctx.framebuffer(w, h), ctx.framebuffer(w, h)
    ctx.render_tiles(fb, w, h, CAP, bounces, tiles, first_pass=0, pass_count=1)
    ctx.copy_framebuffer(fb, half, w, h)
    ctx.render_tiles(fb, w, h, CAP, bounces, tiles, first_pass=1, pass_count=1)
    first, flags = ctx.adaptive_step_cells(fb, half, w, h, tiles, CELL2, INF)
    assert not flags.any() and len(first) == 300
    assert_bit_equal(first, cell_errors(uniform[2], uniform[1], tiles, CELL2), "the measure-only step at 2 passes")
    zero = int((first == 0).sum())
    print(f"{zero} of {len(first)} cells have error exactly 0 at 2 passes")
    assert zero == 92, "input condition: 92 cells' error is exactly 0, so the plain median is too close to 0 to be 'not the uniform frame'; the median of the nonzero ones is used"
    threshold = float(np.median(first[first > 0]))
    out = dict(tiles=tiles, uniform=uniform, first=first, threshold=threshold, bounces=bounces)
    for dilate in (0, 1):
        fb, half = ctx.framebuffer(w, h), ctx.framebuffer(w, h)
        ctx.reset_counters()
        passes, errors = ctx.render_adaptive_cells(fb, half, w, h, CAP, bounces, tiles, min_passes=2, threshold=threshold, cell=CELL2, dilate=dilate)
        ctx.synchronize()
        out[dilate] = dict(passes=passes, errors=errors, paths=ctx.counters()["paths"], fb=fb, half=half, frame=ctx.download(fb, w, h), halfframe=ctx.download(half, w, h))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dilate", [0, 1])
def test_every_cell_of_an_adaptive_frame_is_a_uniform_frame(dilate, pkg, ctx, rendered):
    w, h, R, c = W2, H2, rendered, CELL2
    tiles, uniform, D = R["tiles"], R["uniform"], rendered[dilate]
    passes, errors = D["passes"], D["errors"]
    off = cell_offsets(tiles, c)
    histogram = {n: int((passes == n).sum()) for n in (2, 4, 8, 16)}
    mixed = sum(len(set(passes[off[r]:off[r + 1]].tolist())) > 1 for r in range(len(tiles)))
    print(f"dilate {dilate}, threshold {R['threshold']!r}: cells by pass count {histogram}; {mixed} of {len(tiles)} rectangles hold more than one count")
    assert sum(histogram.values()) == len(passes) == 300
    assert all(histogram.values()), "all four pass counts occur"
    assert mixed >= 1, "some rectangle holds two pass counts"
    want_passes, want_errors = replay(uniform, tiles, c, 2, CAP, R["threshold"], dilate)
    assert np.array_equal(passes, want_passes), np.flatnonzero(passes != want_passes)
    assert_bit_equal(errors, want_errors, "cell errors against the replay")
    k = 0
    for t in tiles:
        for sl in cell_slices(h, t, c):
            n = int(passes[k])
            assert np.array_equal(bits(D["frame"][sl]), bits(uniform[n][sl])), f"cell {k}: the frame is not the uniform {n}-pass frame"
            assert np.array_equal(bits(D["halfframe"][sl]), bits(uniform[n // 2][sl])), f"cell {k}: the half-sample frame is not the uniform {n // 2}-pass frame"
            k += 1
    sizes = np.array([(sl[0].stop - sl[0].start) * (sl[1].stop - sl[1].start) for t in tiles for sl in cell_slices(h, t, c)])
    assert D["paths"] == int((sizes * passes).sum()), "paths = sum of cell pixels x passes"
    counts = pkg.api.sample_count_map_cells(w, h, tiles, c, passes)
    assert counts.dtype == np.int32 and counts.shape == (h, w) and int(counts.sum()) == D["paths"]
    sl = cell_slices(h, tiles[3], c)[5]
    assert (counts[sl] == passes[off[3] + 5]).all()
    if dilate:
        assert not np.array_equal(passes, rendered[0]["passes"]), "dilation changes where the passes go"


# ---- 3. extremes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cell_threshold_extremes(pkg, ctx, rendered):
    """Threshold 0: every cell reaches the cap, the ones whose error at 2 passes is exactly 0 included (without dilation nothing else keeps them going), and the
    frame is the uniform 16-pass frame bit for bit, its half-sample frame the uniform 8-pass one. +inf: every cell stops at min_passes. min_passes = the cap.
    A cell no smaller than the rectangle: one cell each, decided like the rectangle with the 64-lane sum."""
    w, h, R, c = W2, H2, rendered, CELL2
    tiles, uniform, bounces = R["tiles"], R["uniform"], R["bounces"]
    fb, half = ctx.framebuffer(w, h), ctx.framebuffer(w, h)
    for dilate in (0, 1):
        ctx.clear(fb, w, h)
        ctx.clear(half, w, h)
        passes, errors = ctx.render_adaptive_cells(fb, half, w, h, CAP, bounces, tiles, min_passes=2, threshold=0.0, cell=c, dilate=dilate)
        print(f"threshold 0, dilate {dilate}: {int((R['first'] == 0).sum())} cells with error 0 at 2 passes")
        assert (passes == CAP).all(), passes
        same_bits(ctx.download(fb, w, h), uniform[16], "threshold 0: the frame")
        same_bits(ctx.download(half, w, h), uniform[8], "threshold 0: the half-sample frame")
        assert_bit_equal(errors, cell_errors(uniform[16], uniform[8], tiles, c), "threshold 0: errors at the cap")
    ctx.clear(fb, w, h)
    ctx.clear(half, w, h)
    passes, errors = ctx.render_adaptive_cells(fb, half, w, h, CAP, bounces, tiles, min_passes=2, threshold=INF, cell=c, dilate=1)
    assert (passes == 2).all(), passes
    same_bits(ctx.download(fb, w, h), uniform[2], "threshold inf: the frame")
    same_bits(ctx.download(half, w, h), uniform[1], "threshold inf: the half-sample frame")
    assert_bit_equal(errors, R["first"], "threshold inf: errors")
    # min_passes == the cap: one measure-only step
    ctx.clear(fb, w, h)
    passes, _ = ctx.render_adaptive_cells(fb, half, w, h, CAP, bounces, tiles, min_passes=4, threshold=0.0, cell=c, passes=4)
    assert (passes == 4).all()
    same_bits(ctx.download(fb, w, h), uniform[4], "min_passes 4 = cap: the frame")
    same_bits(ctx.download(half, w, h), uniform[2], "min_passes 4 = cap: the half-sample frame")
    # cell >= the rectangle: one cell each; the per-rectangle replay with the 64-lane sum
    H = h
    e = {n: pixel_errors(uniform[n], uniform[n // 2]) for n in (2, 4, 8, 16)}
    rect = lambda n, t: cell_error(e[n][H - t[3]:H - t[1], t[0]:t[2]].ravel())
    at2 = np.array([rect(2, t) for t in tiles], f32)
    assert (at2 > 0).any()
    threshold = float(np.median(at2[at2 > 0]))
    want = []
    for t in tiles:
        n = 2
        while n < CAP and not rect(n, t) <= f32(threshold):
            n *= 2
        want.append(n)
    assert len(set(want)) > 1, "input condition: the rectangles do not all stop at the same count"
    for cell, dilate in ((32, 0), (32, 1), (1024, 1)):
        assert int(pkg.api.adaptive_cell_offsets(tiles, cell)[-1]) == len(tiles)
        ctx.clear(fb, w, h)
        ctx.clear(half, w, h)
        passes, errors = ctx.render_adaptive_cells(fb, half, w, h, CAP, bounces, tiles, min_passes=2, threshold=threshold, cell=cell, dilate=dilate)
        assert passes.tolist() == want, (cell, dilate, passes.tolist(), want)
        assert_bit_equal(errors, np.array([rect(n, t) for n, t in zip(want, tiles)], f32), "one cell a rectangle: errors")


# ---- 4. passes go where the noise is (no renderer) ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", [4, 8, 16])
def test_cells_go_on_where_the_noise_is(c, pkg, ctx):
    w, h = 128, 100
    tiles = grid(pkg, w, h, 32, 20)          # 4 x 5: two columns of rectangles on each side, none straddles the border
    assert all(x1 <= w // 2 or x0 >= w // 2 for x0, y0, x1, y1 in tiles)
    noisy = np.array([sl[1].stop <= w // 2 for t in tiles for sl in cell_slices(h, t, c)])
    fb, half = two_noise_levels(w, h, 8)
    want = cell_errors(fb, half, tiles, c)
    assert noisy.sum() * 2 == len(want)
    lo, hi = float(want[~noisy].max()), float(want[noisy].min())
    print(f"c = {c}: errors of the quiet half up to {lo:.5f}, of the noisy half from {hi:.5f}")
    assert lo < hi, "input condition: the noise levels separate the cells"
    threshold = float(np.sqrt(lo * hi))
    for dilate in (0, 1):
        errors, flags, after = gpu_step_cells(pkg, ctx, fb, half, tiles, c, threshold, dilate)
        assert np.array_equal(flags, noisy), "exactly the cells of the noisy half go on"
        assert_bit_equal(errors, want, f"c = {c}")
        same_bits(after, advance(fb, half, tiles, c, noisy), f"c = {c}: the half-sample frame afterwards")


# ---- 5. composition with the denoiser ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_variance_guided_denoise_of_a_cell_adaptive_frame(pkg, ctx, rendered):
    w, h, D = W2, H2, rendered[1]
    assert len(set(D["passes"].tolist())) > 1
    buf = ctx.aov_buffer(w, h)
    ctx.render_aov(buf, w, h, CAP)
    aov = ctx.download_aov(buf, w, h)
    out = ctx.framebuffer(w, h)
    ctx.denoise_variance(D["fb"], D["half"], buf, w, h, 1, 2, out=out)
    assert_bit_equal(ctx.download(out, w, h), restatement_v(D["frame"], D["halfframe"], aov, 1.0), "denoise_variance of the cell-adaptive frame")
    assert np.array_equal(bits(ctx.download(D["fb"], w, h)), bits(D["frame"])) and np.array_equal(bits(ctx.download(D["half"], w, h)), bits(D["halfframe"]))


# ---- 6. entry points -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cell_entry_point_behaviour(pkg, manifest, golden_blob, tmp_path):
    api, abi = pkg.api, pkg.abi
    L = api.library()
    if api.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device; libcray_hip has no CPU fallback")
    assert abi.ABI_VERSION == 5 and L.crh_abi_version() == 5, "the entry points are additive to ABI 5"
    size, most, version = header_values(tmp_path, "sizeof(crh_adaptive_cells_params)", "CRH_ADAPTIVE_CELLS_MAX", "CRH_ABI_VERSION")
    assert size == C.sizeof(abi.AdaptiveCellsParams) == 16 and most == abi.ADAPTIVE_CELLS_MAX == 1024 and version == 5
    p = abi.AdaptiveCellsParams(-1, -1.0, -1, -1)
    L.crh_adaptive_cells_params_default(C.byref(p))
    assert (p.min_passes, p.threshold, p.cell, p.dilate) == (16, f32(0.05), 16, 1)
    L.crh_adaptive_cells_params_default(None)

    # crh_adaptive_cell_offsets against the formula
    def offsets(tiles_, cell, count=None, out=True):
        arr = (abi.Tile * max(len(tiles_), 1))(*[abi.Tile(*t) for t in tiles_]) if tiles_ is not None else None
        n = (len(tiles_) if count is None else count)
        buf = np.full(n + 1, 0xdeadbeef, np.uint32)
        return L.crh_adaptive_cell_offsets(arr, n, cell, buf.ctypes.data if out else None), buf
    lists = [[(0, 0, 80, 100), (80, 0, 160, 50)], [(3, 5, 4, 6)], [(0, 0, 161, 75), (7, 9, 39, 41), (0, 0, 1, 1000)]]
    for tiles_ in lists:
        for cell in (1, 2, 7, 8, 16, 100, 1024):
            want = [0]
            for x0, y0, x1, y1 in tiles_:
                want.append(want[-1] + ((x1 - x0 + cell - 1) // cell) * ((y1 - y0 + cell - 1) // cell))
            legal = all(b - a <= 1024 for a, b in zip(want, want[1:]))
            total, buf = offsets(tiles_, cell)
            if legal:
                assert total == want[-1] and buf.tolist() == want, (tiles_, cell)
                assert offsets(tiles_, cell, out=False)[0] == total
                assert api.adaptive_cell_offsets(tiles_, cell).tolist() == want
            else:
                assert total == abi.ERR_INVALID and (buf == 0xdeadbeef).all(), (tiles_, cell)
    assert offsets([], 8)[0] == 0 and offsets(None, 8, count=0)[0] == 0
    assert offsets(None, 8, count=2)[0] == abi.ERR_INVALID
    for cell in (0, -1, 1025):
        assert offsets(lists[0], cell)[0] == abi.ERR_INVALID, cell
    assert offsets([(5, 5, 5, 9)], 8)[0] == abi.ERR_INVALID and offsets([(5, 5, 9, 5)], 8)[0] == abi.ERR_INVALID
    assert offsets([(0, 0, 41, 25)], 1)[0] == abi.ERR_INVALID and offsets([(0, 0, 32, 32)], 1)[0] == 1024, "1025 cells are refused, 1024 are not"
    with pytest.raises(api.CrhError):
        api.adaptive_cell_offsets([(0, 0, 41, 25)], 1)

    w, h = 160, 100
    tiles = [(0, 0, 80, 100), (80, 0, 160, 50)]
    cells = int(api.adaptive_cell_offsets(tiles, 16)[-1])
    assert cells == 5 * 7 + 5 * 4
    c = api.Context(0)
    try:
        assert c.adaptive_time_ms() == 0.0
        c.upload(api.Scene(golden_blob("glowmetal")))
        bounces = manifest["glowmetal"]["bounces"]
        fb, half = c.framebuffer(w, h), c.framebuffer(w, h)
        c.render_region(fb, w, h, 2, bounces, first_pass=0, pass_count=1)
        c.copy_framebuffer(fb, half, w, h)
        c.render_region(fb, w, h, 2, bounces, first_pass=1, pass_count=1)
        c.synchronize()
        frame, halfframe = c.download(fb, w, h), c.download(half, w, h)
        before = (c.counters(), c.kernel_time_ms(), c.last_kernel_name())
        errors, flags = np.full(cells, -7.0, np.float32), np.full(cells, 9, np.uint8)

        def untouched(what):
            assert np.array_equal(bits(c.download(fb, w, h)), bits(frame)) and np.array_equal(bits(c.download(half, w, h)), bits(halfframe)), f"{what}: a buffer was written"

        def step(ctxh=c.h, fb_=fb, half_=half, w_=w, h_=h, tiles_=tiles, count=None, cell=16, threshold=0.0, dilate=1, live=None):
            arr = (abi.Tile * max(len(tiles_), 1))(*[abi.Tile(*t) for t in tiles_]) if tiles_ is not None else None
            return L.crh_adaptive_step_cells(ctxh, fb_, half_, w_, h_, arr, len(tiles_) if count is None else count, cell, threshold, dilate,
                                             None if live is None else live.ctypes.data, errors.ctypes.data, flags.ctypes.data)
        assert step(ctxh=None) == abi.ERR_INVALID and step(fb_=None) == abi.ERR_INVALID and step(half_=None) == abi.ERR_INVALID
        assert step(w_=0) == abi.ERR_INVALID and step(h_=-1) == abi.ERR_INVALID
        assert step(tiles_=None, count=2) == abi.ERR_INVALID
        for bad in ((10, 10, 10, 20), (10, 10, 20, 10), (20, 10, 10, 20), (-1, 0, 10, 10), (0, -1, 10, 10), (0, 0, 161, 10), (0, 0, 10, 101)):
            assert step(tiles_=[tiles[0], bad]) == abi.ERR_INVALID, bad
        for bad in (float("nan"), -1.0, -0.0, -INF):
            assert step(threshold=bad) == abi.ERR_INVALID, bad
        assert step(half_=fb) == abi.ERR_INVALID
        for bad in (0, -3, 1025):
            assert step(cell=bad) == abi.ERR_INVALID, bad
        for bad in (-1, 2):
            assert step(dilate=bad) == abi.ERR_INVALID, bad
        assert step(tiles_=[(0, 0, 41, 25)], cell=1) == abi.ERR_INVALID, "a rectangle of 1025 cells"
        assert step(tiles_=[tiles[1], (0, 0, 80, 100)], cell=2) == abi.ERR_INVALID, "a rectangle of 2000 cells behind a legal one"
        assert step(tiles_=[], count=0) == abi.OK and step(tiles_=None, count=0) == abi.OK
        assert (errors == -7.0).all() and (flags == 9).all(), "a refused or empty call writes nothing"
        assert c.adaptive_time_ms() == 0.0, "refused calls are no calls"
        untouched("refused steps")
        # no live cell at all: nothing is launched, the outputs are zeros
        assert step(live=np.zeros(cells, np.uint8)) == abi.OK
        assert (errors == 0).all() and (flags == 0).all() and c.adaptive_time_ms() == 0.0
        untouched("a step with no live cell")
        # NULL result arrays; the step leaves the render path's counters, time and kernel name alone
        assert L.crh_adaptive_step_cells(c.h, fb, half, w, h, (abi.Tile * 2)(*[abi.Tile(*t) for t in tiles]), 2, 16, INF, 1, None, None, None) == abi.OK
        assert step(threshold=INF) == abi.OK
        assert (errors > 0).any() and (flags == 0).all()
        assert c.adaptive_time_ms() > 0.0
        assert (c.counters(), c.kernel_time_ms(), c.last_kernel_name()) == before
        untouched("measure-only steps")
        # a cell step does not change what a following rectangle step returns, and the reverse
        rect_e, rect_f = c.adaptive_step(fb, half, w, h, tiles, INF)
        cell_e, cell_f = c.adaptive_step_cells(fb, half, w, h, tiles, 16, INF, dilate=1)
        again_e, again_f = c.adaptive_step(fb, half, w, h, tiles, INF)
        assert_bit_equal(again_e, rect_e, "a rectangle step behind a cell step")
        assert np.array_equal(again_f, rect_f)
        again_e, again_f = c.adaptive_step_cells(fb, half, w, h, tiles, 16, INF, dilate=1)
        assert_bit_equal(again_e, cell_e, "a cell step behind a rectangle step")
        assert np.array_equal(again_f, cell_f)
        assert_bit_equal(rect_e, restatement(frame, halfframe, tiles, INF)[0], "the rectangle step")
        assert_bit_equal(cell_e, cell_errors(frame, halfframe, tiles, 16), "the cell step")
        with pytest.raises(ValueError):
            c.adaptive_step_cells(fb, half, w, h, tiles, 16, INF, live=np.ones(cells + 1, bool))

        # crh_render_adaptive_cells
        def loop(ctxh=c.h, fb_=fb, half_=half, tiles_=tiles, count=None, min_passes=2, threshold=0.5, cell=16, dilate=1, first_pass=0, cap=16, max_passes=16,
                 null_params=False, null_cells=False):
            q = abi.RenderParams(0, 0, 0, 0, w, h, first_pass, cap, max_passes, bounces)
            a = abi.AdaptiveCellsParams(min_passes, threshold, cell, dilate)
            arr = (abi.Tile * max(len(tiles_), 1))(*[abi.Tile(*t) for t in tiles_]) if tiles_ is not None else None
            return L.crh_render_adaptive_cells(ctxh, None if null_params else C.byref(q), arr, len(tiles_) if count is None else count, None if null_cells else C.byref(a),
                                               fb_, half_, None, None)
        assert loop(ctxh=None) == abi.ERR_INVALID and loop(null_params=True) == abi.ERR_INVALID and loop(null_cells=True) == abi.ERR_INVALID
        assert loop(fb_=None) == abi.ERR_INVALID and loop(half_=None) == abi.ERR_INVALID and loop(half_=fb) == abi.ERR_INVALID
        assert loop(tiles_=None, count=2) == abi.ERR_INVALID and loop(tiles_=[(0, 0, 161, 10)]) == abi.ERR_INVALID and loop(tiles_=[(5, 5, 5, 9)]) == abi.ERR_INVALID
        assert loop(min_passes=3) == abi.ERR_INVALID and loop(min_passes=0) == abi.ERR_INVALID and loop(min_passes=-2) == abi.ERR_INVALID
        assert loop(min_passes=16, cap=24, max_passes=24) == abi.ERR_INVALID, "the cap is not min_passes times a power of two"
        assert loop(min_passes=16, cap=8) == abi.ERR_INVALID and loop(cap=0) == abi.ERR_INVALID
        assert loop(first_pass=1) == abi.ERR_INVALID
        assert loop(cap=16, max_passes=8) == abi.ERR_INVALID, "the cap exceeds max_passes"
        for bad in (float("nan"), -1.0, -0.0):
            assert loop(threshold=bad) == abi.ERR_INVALID, bad
        for bad in (0, -3, 1025):
            assert loop(cell=bad) == abi.ERR_INVALID, bad
        for bad in (-1, 2):
            assert loop(dilate=bad) == abi.ERR_INVALID, bad
        assert loop(tiles_=[(0, 0, 41, 25)], cell=1) == abi.ERR_INVALID, "a rectangle of 1025 cells"
        c.synchronize()
        assert c.counters() == before[0], "a refused render renders nothing"
        untouched("refused renders")
        assert loop(tiles_=[], count=0) == abi.OK and c.counters() == before[0]
        assert loop(threshold=INF, cap=4, max_passes=4) == abi.OK
        c.synchronize()
        assert c.counters()["paths"] == before[0]["paths"] + 2 * (80 * 100 + 80 * 50), "the render dispatches of the loop count like any other"
        with pytest.raises(api.CrhError):
            c.render_adaptive_cells(fb, half, w, h, 24, bounces, tiles)          # the defaults: min_passes 16
        no_scene = api.Context(0)
        try:
            f2, h2 = no_scene.framebuffer(w, h), no_scene.framebuffer(w, h)
            assert loop(ctxh=no_scene.h, fb_=f2, half_=h2) == abi.ERR_INVALID, "no scene uploaded"
        finally:
            no_scene.close()
    finally:
        c.close()


# ---- 7. the drop-in program ------------------------------------------------------------------------------------------------------------------------
def api_threshold_and_frame_cells(pkg, ctx, manifest, golden_blob, tiles, cell, dilate=1):
    """cfg1_scene through the API over `tiles`, min_passes 2 of its 4 samples: the median of the nonzero cell errors of a measure-only step at 2 passes, and
    render_adaptive_cells' frame and pass counts at that threshold."""
    m = manifest["cfg1_scene"]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    assert s == 4
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    fb, half = ctx.framebuffer(w, h), ctx.framebuffer(w, h)
    ctx.render_tiles(fb, w, h, s, b, tiles, first_pass=0, pass_count=1)
    ctx.copy_framebuffer(fb, half, w, h)
    ctx.render_tiles(fb, w, h, s, b, tiles, first_pass=1, pass_count=1)
    first, _ = ctx.adaptive_step_cells(fb, half, w, h, tiles, cell, INF)
    threshold = float(np.median(first[first > 0]))
    ctx.clear(fb, w, h)
    ctx.clear(half, w, h)
    passes, _ = ctx.render_adaptive_cells(fb, half, w, h, s, b, tiles, min_passes=2, threshold=threshold, cell=cell, dilate=dilate)
    assert (passes == 2).any() and (passes == 4).any()
    return threshold, ctx.download(fb, w, h), passes


@pytest.mark.gpu
def test_dropin_program_renders_adaptively_by_cells(pkg, ctx, manifest, golden_blob, tmp_path):
    """c-ray-hip: CRAY_HIP_ADAPTIVE_CELL=16 beside CRAY_HIP_ADAPTIVE writes the frame Context.render_adaptive_cells gives over the scene's tile grid and counts
    cells by pass count; with the variable unset the frame and the image are those of the rectangle-granular loop byte for byte; a value that is no cell size, or a
    rectangle of more than 1024 cells, warns and decides per rectangle."""
    if not dropin_paths()[2]:
        pytest.skip("c-ray-hip or the asset overlay is not built (needs the reference's sources at build time)")
    m = manifest["cfg1_scene"]
    w, h = m["width"], m["height"]
    base = {k: v for k, v in dropin_env().items() if k not in ("CRAY_HIP_ADAPTIVE_CELL", "CRAY_HIP_ADAPTIVE_DILATE")}
    for k in ("CRAY_HIP_ADAPTIVE_CELL", "CRAY_HIP_ADAPTIVE_DILATE"):
        assert k not in os.environ, f"{k} is set in the test's own environment"
    tiles = grid(pkg, w, h, *TILE)
    assert len(tiles) == 25
    # one device, CRAY_HIP_ADAPTIVE_DILATE=0 (the default, 1, is what the two devices below run with)
    threshold, want, passes = api_threshold_and_frame_cells(pkg, ctx, manifest, golden_blob, tiles, 16, 0)
    assert not np.array_equal(passes, api_threshold_and_frame_cells(pkg, ctx, manifest, golden_blob, tiles, 16, 1)[2]), "input condition: dilation changes this frame"
    env = dict(base, CRAY_HIP_ADAPTIVE=repr(threshold), CRAY_HIP_ADAPTIVE_MIN="2", CRAY_HIP_ADAPTIVE_CELL="16", CRAY_HIP_ADAPTIVE_DILATE="0")
    got, files, text = run_dropin(manifest, str(tmp_path / "cells"), env)
    same_bits(got, want, "drop-in against Context.render_adaptive_cells, dilate 0")
    line = [l for l in text.splitlines() if "Adaptive sampling" in l]
    assert len(line) == 1 and f"{len(passes)} cells" in line[0] and "cells of 16" in line[0] and "dilate 0" in line[0], text[-1500:]
    share = 100.0 * float((passes == 2).sum()) / len(passes)
    assert f"2: {share:.1f} %" in line[0] and f"4: {100 - share:.1f} %" in line[0], line
    # unset: the rectangle-granular loop, byte for byte (the frame Context.render_adaptive gives, and the same image whatever CRAY_HIP_ADAPTIVE_DILATE says)
    threshold, want, _ = api_threshold_and_frame(pkg, ctx, manifest, golden_blob, tiles)
    env = dict(base, CRAY_HIP_ADAPTIVE=repr(threshold), CRAY_HIP_ADAPTIVE_MIN="2")
    plain, plain_files, plain_text = run_dropin(manifest, str(tmp_path / "unset"), env)
    same_bits(plain, want, "CRAY_HIP_ADAPTIVE_CELL unset: Context.render_adaptive's frame")
    assert "25 tiles" in plain_text and "cells" not in [l for l in plain_text.splitlines() if "Adaptive sampling" in l][0]
    assert (bits(got) != bits(plain)).any(), "the cell-granular frame is another frame"
    frame, files, text = run_dropin(manifest, str(tmp_path / "bad"), dict(env, CRAY_HIP_ADAPTIVE_CELL="1025"))
    assert "CRAY_HIP_ADAPTIVE_CELL needs" in text and "25 tiles" in text, text[-1500:]
    assert np.array_equal(bits(frame), bits(plain)) and files == plain_files
    frame, files, text = run_dropin(manifest, str(tmp_path / "many"), dict(env, CRAY_HIP_ADAPTIVE_CELL="1"))          # 64 x 40 rectangles: 2560 cells of 1
    assert "deciding per rectangle" in text and "25 tiles" in text, text[-1500:]
    assert np.array_equal(bits(frame), bits(plain)) and files == plain_files
    # two devices, where there are two (the emulation tier has): a share's rectangles are 4-row strips cut every tileWidth columns, so cells are 16 x 4
    if pkg.api.device_count() >= 2:
        tiles = strip_cut_rectangles(w, h, 2)
        threshold, want, passes = api_threshold_and_frame_cells(pkg, ctx, manifest, golden_blob, tiles, 16)
        assert len(passes) == 4 * len(tiles), "cells of 16 x 4: four to a 64-wide strip rectangle"
        got, _, text = run_dropin(manifest, str(tmp_path / "two"), dict(base, CRAY_HIP_DEVICES="2", CRAY_HIP_ADAPTIVE=repr(threshold), CRAY_HIP_ADAPTIVE_MIN="2",
                                                                          CRAY_HIP_ADAPTIVE_CELL="16"))
        same_bits(got, want, "two devices against Context.render_adaptive_cells over the strip-cut rectangles")
        assert f"{len(passes)} cells" in text, text[-1500:]


# ---- 8. the CPU tier ---------------------------------------------------------------------------------------------------------------------------------
def test_adaptive_cells_kernel_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the kernel emulation (tests/emu/libcray_hip_emu.so: k_adaptive_cells and the entry points
    compiled unmodified on the HIP-on-CPU shim, two emulated devices) — every one of them runs and passes there, none skipped (the drop-in test where the drop-in
    program is built)."""
    cases = len(CASES) + 2 + 1 + 3 + 1 + 1          # the step, the uniform-frame test with and without dilation, the extremes, the noise test at three cell sizes, ...
    out = run_gpu_tests_on_emulation(__file__, cases + 1, passed_without_dropin=cases, extra_env={"HIPEMU_DEVICES": "2"}, show_output=True)
    if emulated_dropin():
        assert "two devices against Context.render_adaptive_cells" in out, out[-4000:]
