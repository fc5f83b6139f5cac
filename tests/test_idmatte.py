"""ID mattes (crh_render_ids / crh_ids_resolve / crh_ids_matte, c-ray_amd/csrc/idmatte.h): per pixel, which instances and which materials the camera
rays hit first and how many of the pixel's samples each one got — ranked (id, coverage) pairs, what a compositor isolates an object with.

The result is made of integers, so the GPU tier holds EVERY word of the buffers to a numpy restatement of the header's fold rule over
oracle.camera_ray -> oracle.trace_rays (fields inst and material): both buffers, organic overflow of the six slots, three pass chunks, caller-owned
pre-filled records, every decomposition of a dispatch against one dispatch; in scenes with volumes (which trace_rays refuses) against k_aov's
coverage pass by pass. The two consumers are held bit for bit to numpy float32 restatements. The CPU tier runs this file's GPU tests on the kernel
emulation (tests/emu: the same kernel source on a HIP shim)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import resize_camera
from firsthit_spec import LOST, SLOTS, TOTAL, WORDS, first_hits, ragged_tiles, resolve_expected
from support import EMU_DIR, REPO, DeviceArray, ctx, run_gpu_tests_on_emulation  # noqa: F401 (ctx: the fixture)

SLOT = np.arange(SLOTS)


# ---- the restatements -------------------------------------------------------------------------------------------------------------------
def fold_ids(buf, ids, hit):
    """One sample per pixel into buf [..., 16] uint32 (in place), the header's fold rule: ids [...] uint32, hit [...] bool."""
    idw, cnt = buf[..., 0:SLOTS], buf[..., SLOTS:2 * SLOTS]
    used = (cnt != 0).sum(axis=-1)
    match = (idw == ids[..., None]) & (SLOT < used[..., None]) & hit[..., None]
    match &= np.cumsum(match, axis=-1) == 1                      # the lowest such j
    found = match.any(axis=-1)
    put = (hit & ~found & (used < SLOTS))[..., None] & (SLOT == used[..., None])
    idw[...] = np.where(put, ids[..., None], idw)
    cnt += (match | put).astype(np.uint32)
    buf[..., LOST] += (hit & ~found & (used == SLOTS)).astype(np.uint32)
    buf[..., TOTAL] += np.uint32(1)


def expected_ids(hits, start=None):
    """(instance buffer, material buffer) of the first hits hits[pass][row, col], folded in pass order from `start` (a pair of buffers; None: zeros)."""
    inst = np.zeros(hits.shape[1:] + (WORDS,), np.uint32) if start is None else start[0].copy()
    mat = np.zeros(hits.shape[1:] + (WORDS,), np.uint32) if start is None else start[1].copy()
    for k in range(hits.shape[0]):
        hit = hits[k]["inst"] >= 0
        fold_ids(inst, hits[k]["inst"].astype(np.uint32), hit)
        fold_ids(mat, hits[k]["material"].astype(np.uint32), hit)
    return inst, mat


def matte_expected(buf, ids):
    """crh_ids_matte in numpy float32: [...]."""
    idw, cnt, total = buf[..., 0:SLOTS], buf[..., SLOTS:2 * SLOTS], buf[..., TOTAL]
    member = np.isin(idw, np.array(list(ids), np.uint32)) & (cnt != 0)
    n = np.where(member, cnt, np.uint32(0)).sum(axis=-1, dtype=np.uint32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total != 0, n.astype(np.float32) / total.astype(np.float32), np.float32(0.0)).astype(np.float32)


def used_slots(buf):
    return (buf[..., SLOTS:2 * SLOTS] != 0).sum(axis=-1)


# ---- what the tests share ---------------------------------------------------------------------------------------------------------------
_CASES = {"glowmetal": (160, 100, 5, False), "cfg1_scene": (160, 100, 4, True), "cfg1_tiny": (8, 5, 130, True)}
_cache = {}


def oracle_case(oracle, golden_blob, case):
    """(blob, w, h, passes, resize, hits, (instance buffer, material buffer)) of a case: the oracle's first hits and their fold from zeros, computed once."""
    if case not in _cache:
        w, h, passes, resize = _CASES[case]
        blob = golden_blob("cfg1_scene" if case == "cfg1_tiny" else case)
        oscene = oracle.OracleScene(blob)
        if resize:
            resize_camera(oscene, w, h)
        hits = first_hits(oracle, oscene, w, h, range(passes), passes)
        want = expected_ids(hits)
        for b in want:
            b.setflags(write=False)
        _cache[case] = (blob, w, h, passes, resize, hits, want)
    return _cache[case]


def upload(pkg, ctx, blob, w, h, resize):
    scene = pkg.api.Scene(blob)
    if resize:
        resize_camera(scene, w, h)
    ctx.upload(scene)


def differ(got, want):
    return f"{int((got != want).sum())} words differ"


# ---- the GPU tier -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["glowmetal", "cfg1_scene"])
def test_ids_equal_the_fold_of_the_oracles_first_hits(case, pkg, ctx, oracle, golden_blob):
    """Both buffers of one dispatch over all passes, every word, against the fold rule over the oracle's first hits."""
    blob, w, h, passes, resize, hits, (want_i, want_m) = oracle_case(oracle, golden_blob, case)
    hit_passes = (hits["inst"] >= 0).sum(axis=0)
    ui, um = used_slots(want_i), used_slots(want_m)
    print(f"{case}: {int(((hit_passes > 0) & (hit_passes < passes)).sum())} partially covered pixels, {int((ui == 2).sum())} with two instance ids, "
          f"{int((ui == 3).sum())} with three, {int((ui != um).sum())} where the buffers differ in used slots, {int((hit_passes < passes).sum())} with a miss")
    if case == "glowmetal":
        assert ((hit_passes > 0) & (hit_passes < passes)).sum() >= 200 and (ui == 2).sum() >= 50
    else:
        oscene = oracle.OracleScene(blob)
        assert oscene.desc.instance_count == 19 and (hit_passes == passes).all(), "19 instances, no misses"
        assert (ui == 2).sum() >= 500 and (ui == 3).sum() >= 3 and (ui != um).sum() >= 50
    upload(pkg, ctx, blob, w, h, resize)
    bi, bm = ctx.ids_buffer(w, h), ctx.ids_buffer(w, h)
    ctx.render_ids(bi, bm, w, h, passes)
    got_i, got_m = ctx.download_ids(bi, w, h), ctx.download_ids(bm, w, h)
    assert np.array_equal(got_i, want_i), "instance ids: " + differ(got_i, want_i)
    assert np.array_equal(got_m, want_m), "material ids: " + differ(got_m, want_m)


@pytest.mark.gpu
def test_organic_overflow_and_three_pass_chunks(pkg, ctx, oracle, golden_blob):
    """cfg1_scene at 8 x 5, 130 passes of 130: chunks of 64, 64 and 2 passes, folded by the same lane one after the other; a pixel sees a seventh
    instance and one a seventh material, which `lost` counts."""
    blob, w, h, passes, resize, hits, (want_i, want_m) = oracle_case(oracle, golden_blob, "cfg1_tiny")
    distinct_i = max(len(np.unique(hits["inst"][:, r, c][hits["inst"][:, r, c] >= 0])) for r in range(h) for c in range(w))
    distinct_m = max(len(np.unique(hits["material"][:, r, c][hits["inst"][:, r, c] >= 0])) for r in range(h) for c in range(w))
    print(f"most distinct ids in a pixel: {distinct_i} instances, {distinct_m} materials; lost {int(want_i[..., LOST].sum())} / {int(want_m[..., LOST].sum())}")
    assert distinct_i >= 7 and distinct_m >= 7
    assert want_i[..., LOST].sum() > 0 and want_m[..., LOST].sum() > 0
    upload(pkg, ctx, blob, w, h, resize)
    bi, bm = ctx.ids_buffer(w, h), ctx.ids_buffer(w, h)
    ctx.render_ids(bi, bm, w, h, passes)
    got_i, got_m = ctx.download_ids(bi, w, h), ctx.download_ids(bm, w, h)
    assert np.array_equal(got_i, want_i), "instance ids: " + differ(got_i, want_i)
    assert np.array_equal(got_m, want_m), "material ids: " + differ(got_m, want_m)


@pytest.mark.gpu
def test_caller_owned_prefilled_buffers(pkg, ctx, oracle, golden_blob):
    """A dispatch starts from what the buffer holds: (a) six foreign ids in the slots — every hit is lost; (b) five — the first new id takes slot 5, a second
    one is lost. The reserved words and every pixel outside the rectangle keep their sentinels."""
    blob, w, h, passes, resize, hits, _ = oracle_case(oracle, golden_blob, "glowmetal")
    x0, y0, x1, y1 = region = (23, 11, 90, 58)
    mine = np.s_[h - y1:h - y0, x0:x1]
    sub = hits[:, h - y1:h - y0, x0:x1]
    hit_passes = (sub["inst"] >= 0).sum(axis=0)
    sentinel = (np.arange(w * h * WORDS, dtype=np.uint32) * np.uint32(2654435761) | np.uint32(0x80000000)).reshape(h, w, WORDS)
    upload(pkg, ctx, blob, w, h, resize)
    for filled in (6, 5):
        start = sentinel.copy()
        rec = np.zeros(WORDS, np.uint32)
        rec[0:filled] = 1000 + np.arange(filled)
        rec[SLOTS:SLOTS + filled] = 1 + np.arange(filled)
        rec[TOTAL] = rec[SLOTS:2 * SLOTS].sum()
        start[mine][..., 0:14] = rec[0:14]
        assert rec[TOTAL] == (21 if filled == 6 else 15)
        want_i, want_m = expected_ids(sub, (start[mine], start[mine]))
        if filled == 6:          # every hit goes to lost, the slots are unchanged, total grows by 5
            for want in (want_i, want_m):
                assert np.array_equal(want[..., 0:12], start[mine][..., 0:12]) and np.array_equal(want[..., LOST], hit_passes) and (want[..., TOTAL] == 26).all()
            assert hit_passes.any()
        else:                    # the first new id takes slot 5, a second new id is lost
            first_pass_hit = np.argmax(sub["inst"] >= 0, axis=0)
            first_inst = np.take_along_axis(sub["inst"], first_pass_hit[None], 0)[0]
            some = hit_passes > 0
            assert (want_i[..., 5][some] == first_inst[some].astype(np.uint32)).all() and (want_i[..., 0:5] == rec[0:5]).all()
            assert want_i[..., LOST].sum() > 0 and want_m[..., LOST].sum() > 0, "the rectangle shows pixels with two ids"
            assert np.array_equal(want_i[..., 11] + want_i[..., LOST], hit_passes) and (want_i[..., TOTAL] == 20).all()
        di, dm = DeviceArray(pkg, start, np.uint32), DeviceArray(pkg, start, np.uint32)
        ctx.render_ids(di.ptr, dm.ptr, w, h, passes, region=region)
        for name, dev, want in (("instance", di, want_i), ("material", dm, want_m)):
            got = dev.read(ctx)
            assert np.array_equal(got[mine][..., 0:14], want[..., 0:14]), f"{filled} slots pre-filled, {name} ids: " + differ(got[mine][..., 0:14], want[..., 0:14])
            got[mine][..., 0:14] = sentinel[mine][..., 0:14]
            assert np.array_equal(got, sentinel), "reserved words or pixels outside the rectangle were written"


@pytest.mark.gpu
def test_dispatch_decompositions_give_the_same_buffers(pkg, ctx, oracle, golden_blob):
    blob, w, h, n, resize, _, (want_i, want_m) = oracle_case(oracle, golden_blob, "glowmetal")
    upload(pkg, ctx, blob, w, h, resize)
    bi, bm = ctx.ids_buffer(w, h), ctx.ids_buffer(w, h)
    ctx.render_ids(bi, bm, w, h, n)
    base_i, base_m = ctx.download_ids(bi, w, h), ctx.download_ids(bm, w, h)
    assert np.array_equal(base_i, want_i) and np.array_equal(base_m, want_m)
    # ragged rectangles x consecutive pass ranges
    tiles = ragged_tiles(w, h)
    assert sum((t[2] - t[0]) * (t[3] - t[1]) for t in tiles) == w * h
    ctx.clear_ids(bi, w, h)
    ctx.clear_ids(bm, w, h)
    for first, count in ((0, 1), (1, 3), (4, 1)):
        ctx.render_ids(bi, bm, w, h, n, tiles=tiles, first_pass=first, pass_count=count)
    got_i, got_m = ctx.download_ids(bi, w, h), ctx.download_ids(bm, w, h)
    assert np.array_equal(got_i, base_i) and np.array_equal(got_m, base_m), differ(got_i, base_i) + ", " + differ(got_m, base_m)
    # work units of seven pixel groups (the library sizes them by the dispatch: a frame this small gets units of one group on a full-size GPU)
    ctx.clear_ids(bi, w, h)
    ctx.clear_ids(bm, w, h)
    os.environ["CRH_AOV_UNIT_GROUPS"] = "7"
    try:
        ctx.render_ids(bi, bm, w, h, n, tiles=tiles)
    finally:
        del os.environ["CRH_AOV_UNIT_GROUPS"]
    got_i, got_m = ctx.download_ids(bi, w, h), ctx.download_ids(bm, w, h)
    assert np.array_equal(got_i, base_i) and np.array_equal(got_m, base_m), differ(got_i, base_i) + ", " + differ(got_m, base_m)
    # one buffer alone gets the words it gets in the joint dispatch
    ctx.clear_ids(bi, w, h)
    ctx.clear_ids(bm, w, h)
    ctx.render_ids(bi, None, w, h, n)
    ctx.render_ids(None, bm, w, h, n)
    got_i, got_m = ctx.download_ids(bi, w, h), ctx.download_ids(bm, w, h)
    assert np.array_equal(got_i, base_i) and np.array_equal(got_m, base_m), differ(got_i, base_i) + ", " + differ(got_m, base_m)
    # a single pixel
    x, y = 75, 42
    ctx.clear_ids(bi, w, h)
    ctx.clear_ids(bm, w, h)
    ctx.render_ids(bi, bm, w, h, n, region=(x, y, x + 1, y + 1))
    for got, base in ((ctx.download_ids(bi, w, h), base_i), (ctx.download_ids(bm, w, h), base_m)):
        assert np.array_equal(got[h - 1 - y, x], base[h - 1 - y, x]) and got[h - 1 - y, x, SLOTS] > 0
        got[h - 1 - y, x] = 0
        assert not got.any()


@pytest.mark.gpu
@pytest.mark.parametrize("halton", [False, True], ids=["random", "halton"])
def test_volumes_and_the_halton_sampler_against_the_aov_coverage(halton, pkg, ctx, oracle, golden_blob):
    """trace_rays refuses volumes, so the yardstick is k_aov: one render_aov per pass into a cleared buffer says which passes of a pixel hit."""
    name, w, h, passes = "volumes", 240, 160, 8
    blob = golden_blob(name)
    oscene = oracle.OracleScene(blob)
    d = oscene.desc
    volume_instances = [i for i in range(d.instance_count) if d.instances[i].kind in (2, 3)]          # CRH_INSTANCE_SPHERE_VOLUME, CRH_INSTANCE_MESH_VOLUME
    assert volume_instances
    upload(pkg, ctx, blob, w, h, False)
    ctx.set_option(pkg.abi.OPT_SAMPLER, pkg.abi.SAMPLER_HALTON if halton else pkg.abi.SAMPLER_RANDOM)
    try:
        aov = ctx.aov_buffer(w, h)
        hit_passes = np.zeros((h, w), np.uint32)
        for p in range(passes):
            ctx.clear_aov(aov, w, h)
            ctx.render_aov(aov, w, h, passes, first_pass=p, pass_count=1)
            hit_passes += (ctx.download_aov(aov, w, h)[..., 7] > 0).astype(np.uint32)
        bi, bm = ctx.ids_buffer(w, h), ctx.ids_buffer(w, h)
        ctx.render_ids(bi, bm, w, h, passes)
        got_i, got_m = ctx.download_ids(bi, w, h), ctx.download_ids(bm, w, h)
    finally:
        ctx.set_option(pkg.abi.OPT_SAMPLER, pkg.abi.SAMPLER_RANDOM)
    partial = int(((hit_passes > 0) & (hit_passes < passes)).sum())
    print(f"{name} {'halton' if halton else 'random'}: {partial} partially covered pixels")
    assert partial >= 100
    for got, limit in ((got_i, d.instance_count), (got_m, d.material_count)):
        cnt = got[..., SLOTS:2 * SLOTS]
        assert np.array_equal(cnt.sum(axis=-1, dtype=np.uint32) + got[..., LOST], hit_passes)
        assert (got[..., TOTAL] == passes).all() and not got[..., 14:16].any()
        assert (got[..., 0:SLOTS][cnt != 0] < limit).all() and not got[..., 0:SLOTS][cnt == 0].any()
        used = used_slots(got)
        assert ((cnt != 0) == (SLOT < used[..., None])).all(), "slots fill front to back"
    in_volume = np.isin(got_i[..., 0:SLOTS], volume_instances) & (got_i[..., SLOTS:2 * SLOTS] != 0)
    print(f"{int(in_volume.any(axis=-1).sum())} pixels hold a volume's instance")
    assert in_volume.any()


def synthetic_buffer():
    """Caller-filled records: equal counts in several slots, empty slots, a full record, total == 0, ids and counts beyond 2^24, and random valid ones."""
    rng = np.random.default_rng(20261019)
    hnd = [
        ([7, 3, 9, 0, 0, 0], [4, 4, 4, 0, 0, 0], 0, 16),                            # equal counts: the lower slot first
        ([7, 3, 9, 11, 2, 5], [1, 6, 6, 2, 6, 1], 3, 25),                           # a full record with ties and lost samples
        ([0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], 0, 0),                             # nothing
        ([0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], 0, 9),                             # nine misses
        ([5, 6, 0, 0, 0, 0], [3, 1, 0, 0, 0, 0], 0, 0),                             # total == 0: all empty ranks, matte 0
        ([0, 4, 0, 0, 0, 0], [2, 5, 0, 0, 0, 0], 0, 7),                             # id 0 in a used slot
        ([16777217, 4294967295, 33554435, 0, 0, 0], [16777217, 3, 1, 0, 0, 0], 0, 16777221),          # ids and counts that round in the conversion
        ([1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6], 0, 21),                            # ascending counts: the network reverses them
        ([1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1], 0, 21),
        ([1, 2, 3, 4, 5, 6], [2, 2, 2, 2, 2, 2], 7, 19),
    ]
    h, w = 7, 9
    buf = np.zeros((h, w, WORDS), np.uint32)
    flat = buf.reshape(-1, WORDS)
    for k, (ids, cnt, lost, total) in enumerate(hnd):
        flat[k, 0:SLOTS], flat[k, SLOTS:2 * SLOTS], flat[k, LOST], flat[k, TOTAL] = ids, cnt, lost, total
    for k in range(len(hnd), h * w):
        used = int(rng.integers(0, SLOTS + 1))
        flat[k, 0:used] = rng.permutation(12)[:used]
        flat[k, SLOTS:SLOTS + used] = rng.integers(1, 4, used)          # few values: many ties
        flat[k, LOST] = rng.integers(0, 3) if used == SLOTS else 0
        flat[k, TOTAL] = flat[k, SLOTS:2 * SLOTS].sum() + flat[k, LOST] + rng.integers(0, 5)
    flat[:, 14:16] = 0xDEADBEEF
    return buf


@pytest.mark.gpu
def test_resolve_and_matte_equal_their_restatements(pkg, ctx, oracle, golden_blob):
    """Ranked pairs and mattes of the buffers the dispatch tests hold to the oracle and of a caller-filled buffer, bit for bit; no scene is involved."""
    inputs = [("synthetic", synthetic_buffer(), None)]
    for case in ("glowmetal", "cfg1_scene", "cfg1_tiny"):
        _, w, h, passes, _, hits, (want_i, want_m) = oracle_case(oracle, golden_blob, case)
        inputs += [(case + " instances", want_i, hits), (case + " materials", want_m, None)]
    ties = 0
    for name, buf, hits in inputs:
        h, w = buf.shape[:2]
        dev = DeviceArray(pkg, buf, np.uint32)
        out = DeviceArray(pkg, np.full((h, w, SLOTS, 2), 7.0, np.float32))
        ctx.resolve_ids(dev.ptr, w, h, out.ptr)
        got, want = out.read(ctx), resolve_expected(buf)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{name}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} floats of the ranking differ"
        cnt = buf[..., SLOTS:2 * SLOTS]
        ties += int(((cnt[..., :-1] == cnt[..., 1:]) & (cnt[..., 1:] != 0)).any(axis=-1).sum())
        present = np.unique(buf[..., 0:SLOTS][cnt != 0])
        mout = DeviceArray(pkg, np.full((h, w), 7.0, np.float32))
        lists = [[], [int(present[0])], [int(present[0])] * 3, [int(i) for i in present[:2]] + [int(present[0])], [int(i) for i in present[-64:]], [4000000000]]
        mattes = []
        for ids in lists:
            ctx.ids_matte(dev.ptr, w, h, ids, mout.ptr)
            got, want = mout.read(ctx), matte_expected(buf, ids)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{name}, ids {ids[:4]}...: {int((got != want).sum())} floats of the matte differ"
            mattes.append(got)
        assert not mattes[0].any() and not mattes[5].any(), "an empty list, and an id no pixel holds, give zeros"
        assert np.array_equal(mattes[1], mattes[2]) and mattes[1].any(), "a duplicate id changes nothing"
        assert np.array_equal(mattes[3], matte_expected(buf, lists[3][:2]))
        assert np.array_equal(dev.read(ctx), buf), "the consumers do not write the ID buffer"
        if hits is not None:          # all the ids of the buffer: what is left of a pixel is its lost samples and its misses
            assert len(present) <= 64
            misses = (hits["inst"] < 0).sum(axis=0).astype(np.uint32)
            total = buf[..., TOTAL]
            assert np.array_equal(cnt.sum(axis=-1, dtype=np.uint32) + buf[..., LOST] + misses, total)
            want = ((total - buf[..., LOST] - misses).astype(np.float32) / total.astype(np.float32)).astype(np.float32)
            assert np.array_equal(mattes[4].view(np.uint32), want.view(np.uint32))
    print(f"{ties} pixels with equal counts in neighbouring used slots")
    assert ties >= 3          # (three of the hand-written records tie by construction)


@pytest.mark.gpu
def test_entry_point_behaviour(pkg, golden_blob):
    api, abi = pkg.api, pkg.abi
    L = api.library()
    if api.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device; libcray_hip has no CPU fallback")
    w, h = 160, 100
    c = api.Context(0)
    try:
        bi, bm = c.ids_buffer(w, h), c.ids_buffer(w, h)
        p = abi.RenderParams(0, 0, w, h, w, h, 0, 2, 2, 0)
        assert c.ids_kernel_time_ms() == 0.0
        assert L.crh_render_ids(c.h, C.byref(p), None, 0, bi, bm) == abi.ERR_INVALID          # no scene
        # the consumers need none
        out = DeviceArray(pkg, np.full((h, w, SLOTS, 2), 7.0, np.float32))
        mout = DeviceArray(pkg, np.full((h, w), 7.0, np.float32))
        c.resolve_ids(bi, w, h, out.ptr)
        c.ids_matte(bi, w, h, [0, 1], mout.ptr)
        got = out.read(c)
        assert (got[..., 0] == -1.0).all() and not got[..., 1].any() and not mout.read(c).any()
        assert c.ids_kernel_time_ms() > 0.0
        ids = (C.c_uint32 * 65)(*range(65))
        assert L.crh_ids_matte(c.h, bi, w, h, ids, 65, mout.ptr) == abi.ERR_INVALID             # more than CRH_IDS_MATTE_MAX
        assert L.crh_ids_matte(c.h, bi, w, h, None, 1, mout.ptr) == abi.ERR_INVALID             # a count without a list
        assert L.crh_ids_matte(c.h, bi, w, h, ids, 64, mout.ptr) == abi.OK
        assert L.crh_ids_matte(c.h, bi, w, h, None, 0, mout.ptr) == abi.OK
        assert L.crh_ids_matte(None, bi, w, h, ids, 1, mout.ptr) == abi.ERR_INVALID
        assert L.crh_ids_matte(c.h, None, w, h, ids, 1, mout.ptr) == abi.ERR_INVALID
        assert L.crh_ids_matte(c.h, bi, w, h, ids, 1, None) == abi.ERR_INVALID
        assert L.crh_ids_matte(c.h, bi, 0, h, ids, 1, mout.ptr) == abi.ERR_INVALID
        assert L.crh_ids_resolve(None, bi, w, h, out.ptr) == abi.ERR_INVALID
        assert L.crh_ids_resolve(c.h, None, w, h, out.ptr) == abi.ERR_INVALID
        assert L.crh_ids_resolve(c.h, bi, w, h, None) == abi.ERR_INVALID
        assert L.crh_ids_resolve(c.h, bi, w, -1, out.ptr) == abi.ERR_INVALID
        c.upload(api.Scene(golden_blob("glowmetal")))
        ptr = C.c_void_p()
        assert L.crh_ids_alloc(None, w, h, C.byref(ptr)) == abi.ERR_INVALID
        assert L.crh_ids_alloc(c.h, w, h, None) == abi.ERR_INVALID
        assert L.crh_ids_alloc(c.h, 0, h, C.byref(ptr)) == abi.ERR_INVALID
        assert L.crh_ids_free(None, None) == abi.ERR_INVALID
        assert L.crh_ids_clear(c.h, None, w, h) == abi.ERR_INVALID
        assert L.crh_ids_download(c.h, bi, w, h, None) == abi.ERR_INVALID
        assert L.crh_ids_download(c.h, None, w, h, None) == abi.ERR_INVALID
        assert L.crh_ids_kernel_time_ms(c.h, None) == abi.ERR_INVALID
        assert L.crh_render_ids(None, C.byref(p), None, 0, bi, bm) == abi.ERR_INVALID
        assert L.crh_render_ids(c.h, None, None, 0, bi, bm) == abi.ERR_INVALID
        assert L.crh_render_ids(c.h, C.byref(p), None, 0, None, None) == abi.ERR_INVALID        # both buffers NULL
        assert L.crh_render_ids(c.h, C.byref(p), None, 0, bi, bi) == abi.ERR_INVALID            # the two buffers equal
        assert L.crh_render_ids(c.h, C.byref(p), None, 3, bi, bm) == abi.ERR_INVALID            # a count without a list
        for bad in ((0, 0, w + 1, h), (-1, 0, w, h), (0, 0, w, h + 1), (0, -2, w, h)):
            with pytest.raises(api.CrhError) as e:
                c.render_ids(bi, bm, w, h, 2, region=bad)
            assert e.value.code == abi.ERR_INVALID
            with pytest.raises(api.CrhError) as e:
                c.render_ids(bi, None, w, h, 2, tiles=[(0, 0, 4, 4), bad])
            assert e.value.code == abi.ERR_INVALID
        with pytest.raises(api.CrhError) as e:
            c.render_ids(bi, bm, w, h, 2, first_pass=1, pass_count=2)                          # passes beyond max_passes
        assert e.value.code == abi.ERR_INVALID
        # dispatches without work: CRH_OK, nothing written
        c.render_ids(bi, bm, w, h, 2, pass_count=0)
        c.render_ids(bi, bm, w, h, 2, region=(5, 5, 5, 9))
        c.render_ids(bi, bm, w, h, 2, tiles=[])
        c.render_ids(bi, bm, w, h, 2, tiles=[(3, 3, 3, 3), (9, 4, 12, 4)])
        assert not c.download_ids(bi, w, h).any() and not c.download_ids(bm, w, h).any()
        # the render path's counters, time and kernel name are the render's after the ID kernels
        fb = c.framebuffer(w, h)
        c.reset_counters()
        c.render_region(fb, w, h, 2, 3)
        before = (c.counters(), c.kernel_time_ms(), c.last_kernel_name())
        c.render_ids(bi, bm, w, h, 2)
        c.resolve_ids(bi, w, h, out.ptr)
        c.ids_matte(bm, w, h, [0], mout.ptr)
        got = c.download_ids(bi, w, h)
        assert (c.counters(), c.kernel_time_ms(), c.last_kernel_name()) == before
        assert got[..., SLOTS].any() and (got[..., TOTAL] == 2).all() and c.ids_kernel_time_ms() > 0.0
        c.clear_ids(bi, w, h)
        assert not c.download_ids(bi, w, h).any()
    finally:
        c.close()


# ---- the CPU tier -----------------------------------------------------------------------------------------------------------------------
def test_id_kernels_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the kernel emulation (tests/emu/libcray_hip_emu.so: k_ids, the two consumers and their
    entry points compiled unmodified on the HIP-on-CPU shim) — every one of them runs and passes there, none skipped."""
    run_gpu_tests_on_emulation(__file__, 9)
    header, obj = os.path.join(REPO, "c-ray_amd", "csrc", "idmatte.h"), os.path.join(EMU_DIR, "_obj", "kernel_emu.o")
    assert os.path.getmtime(header) <= os.path.getmtime(obj), "the emulation's kernel object is older than csrc/idmatte.h"
