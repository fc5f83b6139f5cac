"""The rolling kernel's cheaper steps (round 10: c-ray_amd/csrc/cray_hip.hip, CRH_MERGED_ADVANCE / CRH_WAVE_SCOPE_FENCE / CRH_STEP_ARGS) render the same frames.

The node run of k_pathtrace_roll advances its node lanes and its triangle lanes at ONE site, its per-wave steps end in a wavefront-scope fence, and its SHADE and
MISS steps read the shading tables' addresses and counts from a record in memory instead of from kernel arguments. No step moves and no scheduling decision changes
(tests/test_kernel_emu.py pins the step counts); these are the smallest inputs on which each of the three could go wrong, every one against the oracle, bit for bit,
with equal ray, node-test and triangle-test counts:

  1. many small mesh instances under one top level, with tri_in_run = ctrl_in_run = 1: node, triangle and control lanes are served in the same iteration of a node
     run, and BLAS leaves from node steps and from triangle steps coincide — the merged advance;
  2. more materials than CRH_SHADE_LDS_MATERIALS, more images than CRH_SHADE_LDS_IMAGES (every shading table comes from global memory, through the record), and a
     scene of one material (the LDS copies, staged through the record);
  3. a job ring that wraps: two ragged tiles, 9 passes in chunks of 2, units of a few pixels — several chunks per unit, FOLD and OPEN right behind SHADE and MISS —
     with the rolling kernel and, where the library holds it (the emulation tier), the one-unit-at-a-time form.

The walk counts are compared under CRH_OPT_RENDER_SLABS = LITERAL, where the walk is the reference's node for node; the default slab test must
give the same frame and the same rays. GPU tier: -m gpu. CPU tier: the same tests on the kernel emulation (tests/emu).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import kernel_forms
from scene_synth import DIFFUSE, IMAGE_NO_BILINEAR, MIX, SynthScene
from support import ctx, run_gpu_tests_on_emulation  # noqa: F401 (ctx: the fixture)

SHADE_LDS_MATERIALS, SHADE_LDS_IMAGES = 24, 8          # CRH_SHADE_LDS_MATERIALS, CRH_SHADE_LDS_IMAGES (c-ray_amd/csrc/cray_hip.hip)
SCHED = (70, 160, 120, 16)                             # the scheduler weights every test of the suite restores (tests/test_gpu_parity.py)
SIZE, SPP, BOUNCES = 64, 4, 4


def centre_region(w, h, rw=SIZE, rh=SIZE):
    x0, y0 = (w - rw) // 2, (h - rh) // 2
    return (x0, y0, x0 + rw, y0 + rh)


def against_oracle(pkg, ctx, oracle, scene, w, h, spp, bounces, tiles, what):
    """The tiles on the device (one dispatch) and with the oracle, under both slab tests: equal frames bit for bit, nothing outside the tiles touched, equal ray and
    path counts; with the literal slab test equal node-test and triangle-test counts as well."""
    abi = pkg.abi
    ref = np.zeros((h, w, 3), np.float32)
    want = dict(rays=0, node_tests=0, tri_tests=0, paths=0)
    inside = np.zeros((h, w), bool)
    for t in tiles:
        _, ocnt = oracle.render(scene, w, h, spp, bounces, region=t, fb=ref, threads=2)
        for k in want:
            want[k] += ocnt[k]
        inside[h - t[3]:h - t[1], t[0]:t[2]] = True
    ctx.upload(scene)
    fb = ctx.framebuffer(w, h)
    try:
        for slabs in (abi.TRACE_SLABS_EXACT, abi.TRACE_SLABS_LITERAL):
            ctx.set_option(abi.OPT_RENDER_SLABS, slabs)
            ctx.clear(fb, w, h)
            ctx.reset_counters()
            ctx.render_tiles(fb, w, h, spp, bounces, tiles)
            img, cnt = ctx.download(fb, w, h), ctx.counters()
            differ = int((img.view(np.uint32) != ref.view(np.uint32)).sum())
            print(f"{what} (slabs {slabs}, {ctx.last_kernel_name()}): {differ} floats differ; rays {cnt['rays']} / {want['rays']}, node tests {cnt['node_tests']} / "
                  f"{want['node_tests']}, triangle tests {cnt['tri_tests']} / {want['tri_tests']}")
            assert differ == 0, (what, slabs, differ)
            assert not img[~inside].any(), what
            assert cnt["rays"] == want["rays"] and cnt["paths"] == want["paths"] == int(inside.sum()) * spp, (what, slabs, cnt, want)
            if slabs == abi.TRACE_SLABS_LITERAL:
                assert cnt["node_tests"] == want["node_tests"] and cnt["tri_tests"] == want["tri_tests"], (what, cnt, want)
    finally:
        ctx.set_option(abi.OPT_RENDER_SLABS, abi.TRACE_SLABS_EXACT)
    return ref, want


# ---- 1. many small mesh instances ------------------------------------------------------------------------------------------------------------
def affine(m3, t):
    """(A, Ainv) of x -> m3 x + t as the 12 floats of a crh_instance each (row-major 3 x 4)."""
    m3, t = np.asarray(m3, np.float64), np.asarray(t, np.float64)
    inv = np.linalg.inv(m3)
    return (np.hstack([m3, t[:, None]]).astype(np.float32).ravel(), np.hstack([inv, (-inv @ t)[:, None]]).astype(np.float32).ravel())


def instance_bounds(d, inst):
    """World-space box of an instance: the corners of its object's box (a mesh's root node, a sphere's radius) through A, with a margin."""
    if inst.kind == 1:
        b = list(d.nodes[d.meshes[inst.object].node_base].bounds)
    else:
        r = d.spheres[inst.object].radius
        b = [-r, r, -r, r, -r, r]
    A = np.array(list(inst.A), np.float64).reshape(3, 4)
    corners = np.array([[b[i], b[2 + j], b[4 + k], 1.0] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    p = corners @ A.T
    lo, hi = p.min(axis=0), p.max(axis=0)
    pad = 1e-3 * (1.0 + np.abs(p).max())
    return lo - pad, hi + pad


def top_level(boxes):
    """A binary BVH over the boxes in crh_bvh_node form: median split of the centres along their widest axis, leaves of at most two; children of an inner node are the
    nodes first, first + 1, a leaf names entries first .. first + count of the order. Returns (node records, order)."""
    nodes, order = [None], []

    def fill(ni, ids):
        lo = np.min([boxes[i][0] for i in ids], axis=0)
        hi = np.max([boxes[i][1] for i in ids], axis=0)
        bounds = (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])
        if len(ids) <= 2:
            nodes[ni] = (bounds, len(order), len(ids) | (1 << 30))
            order.extend(ids)
            return
        centres = np.array([(boxes[i][0] + boxes[i][1]) / 2 for i in ids])
        axis = int(np.argmax(centres.max(axis=0) - centres.min(axis=0)))
        ids = [ids[k] for k in np.argsort(centres[:, axis], kind="stable")]
        first = len(nodes)
        nodes.extend([None, None])
        nodes[ni] = (bounds, first, 0)
        fill(first, ids[:len(ids) // 2])
        fill(first + 1, ids[len(ids) // 2:])

    fill(0, list(range(len(boxes))))
    return nodes, order


def many_small_instances(oracle, blob, w, h, region, columns=8, rows=5):
    """cfg1_scene with columns x rows more mesh instances — its two-triangle quad and its twelve-triangle box, shrunk, alternating — spread over what the region's
    camera rays see a little in front of the camera, and a top-level BVH rebuilt over all instances (the BLASes stay the reference builder's)."""
    abi = oracle.abi
    base = oracle.OracleScene(blob)
    s = SynthScene(base)
    d = s.desc
    assert d.tlas_node_base + d.tlas_node_count == d.node_count and d.tlas_prim_base + d.tlas_prim_count == d.prim_index_count          # the TLAS lies behind the BLASes
    quad = next(i for i in range(d.instance_count) if d.instances[i].kind == 1 and d.meshes[d.instances[i].object].poly_count == 2)
    box = next(i for i in range(d.instance_count) if d.instances[i].kind == 1 and 2 < d.meshes[d.instances[i].object].poly_count <= 16)
    bb = list(d.nodes[d.meshes[d.instances[box].object].node_base].bounds)
    box_centre, box_width = np.array([(bb[0] + bb[1]) / 2, (bb[2] + bb[3]) / 2, (bb[4] + bb[5]) / 2]), bb[1] - bb[0]
    # where the corner rays of the region are at depth z: in front of everything the scene's own instances show there
    z = 740.0

    def at_depth(x, y, depth):
        r = np.asarray(oracle.camera_ray(base, x, y, 0, 1), np.float64)
        return r[0:3] + r[3:6] * ((depth - r[2]) / r[5])
    x0, y0, x1, y1 = region
    c00, c10, c01, c11 = at_depth(x0, y0, z), at_depth(x1 - 1, y0, z), at_depth(x0, y1 - 1, z), at_depth(x1 - 1, y1 - 1, z)
    spacing = float(np.linalg.norm(c10 - c00)) / columns
    n0 = d.instance_count
    count = columns * rows
    inst = s._array("instances", extra=count)
    for k in range(count):
        i, j = k % columns, k // columns
        u, v = (i + 0.5) / columns, (j + 0.5) / rows
        p = (1 - u) * (1 - v) * c00 + u * (1 - v) * c10 + (1 - u) * v * c01 + u * v * c11
        p[2] += 10.0 * ((k * 3) % 7)          # staggered in depth: neighbours overlap on the screen
        if k % 2 == 0:          # the quad lies in its xz plane: stood up to face the camera, two spacings wide
            e = 2.0 * spacing
            src, (A, Ainv) = quad, affine([[e, 0, 0], [0, 0, e], [0, -e, 0]], p)
        else:
            e = 2.0 * spacing / box_width
            src, (A, Ainv) = box, affine(np.eye(3) * e, p - e * box_centre)
        C.memmove(C.byref(inst[n0 + k]), C.byref(inst[src]), C.sizeof(abi.Instance))
        for q in range(12):
            inst[n0 + k].A[q], inst[n0 + k].Ainv[q] = float(A[q]), float(Ainv[q])
    total = n0 + count
    nodes, order = top_level([instance_bounds(d, inst[i]) for i in range(total)])
    node_arr = (abi.BvhNode * (d.tlas_node_base + len(nodes)))()
    C.memmove(node_arr, d.nodes, d.tlas_node_base * C.sizeof(abi.BvhNode))
    for k, (bounds, first, count_leaf) in enumerate(nodes):
        n = node_arr[d.tlas_node_base + k]
        for q in range(6):
            n.bounds[q] = float(np.float32(bounds[q]))
        n.first, n.count_leaf = first, count_leaf
    prim_arr = (C.c_int32 * (d.tlas_prim_base + total))()
    C.memmove(prim_arr, d.prim_indices, d.tlas_prim_base * 4)
    for k, i in enumerate(order):
        prim_arr[d.tlas_prim_base + k] = i
    s._own["nodes"], s._own["prim_indices"] = node_arr, prim_arr          # (kept alive with the description)
    d.nodes, d.node_count = C.cast(node_arr, C.POINTER(abi.BvhNode)), len(node_arr)
    d.prim_indices, d.prim_index_count = C.cast(prim_arr, C.POINTER(C.c_int32)), len(prim_arr)
    d.tlas_node_count, d.tlas_prim_count = len(nodes), total
    return s, count


@pytest.mark.gpu
def test_many_small_instances_with_every_step_kind_in_the_run(pkg, ctx, oracle, manifest, golden_blob):
    """64 x 64 pixels, 4 spp, 4 bounces over 40 shrunken quads and boxes in front of cfg1_scene, with tri_in_run = ctrl_in_run = 1: every iteration of a node run serves
    its triangle lanes and its control lanes too, so node steps and triangle steps leave BLASes in the same iteration and both go through the one advance site."""
    m = manifest["cfg1_scene"]
    w, h = m["width"], m["height"]
    region = centre_region(w, h)
    scene, added = many_small_instances(oracle, golden_blob("cfg1_scene"), w, h, region)
    assert added == 40 and scene.desc.instance_count == 59
    plain, _ = oracle.render(oracle.OracleScene(golden_blob("cfg1_scene")), w, h, SPP, BOUNCES, region=region, threads=2)
    try:
        ctx.set_sched(*SCHED, tri_in_run=1, ctrl_in_run=1)
        ref, want = against_oracle(pkg, ctx, oracle, scene, w, h, SPP, BOUNCES, [region], "40 small instances, tri_in_run = ctrl_in_run = 1")
        ctx.set_sched(*SCHED)
        against_oracle(pkg, ctx, oracle, scene, w, h, SPP, BOUNCES, [region], "40 small instances, default thresholds")
    finally:
        ctx.set_sched(*SCHED)
    assert ",false," in ctx.last_kernel_name() and "k_pathtrace_roll" in ctx.last_kernel_name(), ctx.last_kernel_name()
    x0, y0, x1, y1 = region
    changed = float((ref != plain).any(axis=2)[h - y1:h - y0, x0:x1].mean())
    print(f"pixels of the region that the added instances change: {changed:.2f}; triangle tests {want['tri_tests']}")
    assert changed > 0.5 and want["tri_tests"] > 4 * SIZE * SIZE * SPP, (changed, want)          # the instances are what the region shows


# ---- 2. the shading tables in global memory and in LDS -------------------------------------------------------------------------------------------
def with_many_materials(oracle, blob):
    """fence with 20 more diffuse materials (33 > CRH_SHADE_LDS_MATERIALS), six of them on its spheres."""
    s = SynthScene(oracle.OracleScene(blob))
    mats = [s.material(s.bsdf(DIFFUSE, s.color(0.15 + 0.04 * k, 0.9 - 0.035 * k, 0.2 + 0.03 * ((k * 7) % 11)))) for k in range(20)]
    for k in range(s.desc.sphere_count):
        s.set_sphere_material(k, mats[(3 * k) % len(mats)])
    return s


def with_many_images(oracle, blob):
    """fence with twelve 3 x 2 textures behind twelve image nodes (> CRH_SHADE_LDS_IMAGES), two of them mixed in each sphere's material."""
    s = SynthScene(oracle.OracleScene(blob))
    rng = np.random.default_rng(10)
    images = [s.image(s.texture(rng.integers(0, 256, (2, 3, 3), dtype=np.uint8)), IMAGE_NO_BILINEAR if k % 2 else 0) for k in range(12)]
    for k in range(s.desc.sphere_count):
        a, b = s.bsdf(DIFFUSE, images[(2 * k) % 12]), s.bsdf(DIFFUSE, images[(2 * k + 1) % 12])
        s.set_sphere_material(k, s.material(s.bsdf(MIX, a, b, s.value(0.5))))
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["materials", "images", "one_material"])
def test_shading_tables_from_the_record(case, pkg, ctx, oracle, manifest, golden_blob):
    """64 x 64 pixels, 4 spp, 4 bounces. materials / images: a table too long for its LDS copy, so SHADE and MISS read every table from global memory at the
    addresses the record holds. one_material: uvsphere, whose tables are staged in LDS — from the record's addresses and counts — at the start of the kernel."""
    name = "uvsphere" if case == "one_material" else "fence"
    m = manifest[name]
    w, h = m["width"], m["height"]
    if case == "materials":
        scene = with_many_materials(oracle, golden_blob(name))
        assert scene.desc.material_count > SHADE_LDS_MATERIALS
    elif case == "images":
        scene = with_many_images(oracle, golden_blob(name))
        assert scene.desc.texture_count > SHADE_LDS_IMAGES
    else:
        scene = oracle.OracleScene(golden_blob(name))
        assert scene.desc.material_count == 1
    ref, _ = against_oracle(pkg, ctx, oracle, scene, w, h, SPP, BOUNCES, [centre_region(w, h)], case)
    assert ",false," in ctx.last_kernel_name(), ctx.last_kernel_name()          # the lean instantiation: no node programs in these graphs
    assert ref.any()


# ---- 3. a job ring that wraps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_job_ring_wraps_with_ragged_chunks(pkg, ctx, oracle, manifest, golden_blob):
    """48 x 40 pixels of fence in two tiles of 29 and 19 columns, 9 passes in chunks of 2 (the last chunk is one pass), units of 64 items: every unit is several jobs,
    a wave's four slots are reused many times, and FOLD / OPEN follow SHADE and MISS at once. Every kernel form the library holds must give the oracle's frame."""
    abi = pkg.abi
    m = manifest["fence"]
    w, h = m["width"], m["height"]
    x0, y0 = (w - 48) // 2, (h - 40) // 2
    tiles = [(x0, y0, x0 + 29, y0 + 40), (x0 + 29, y0, x0 + 48, y0 + 40)]
    scene = oracle.OracleScene(golden_blob("fence"))
    forms = kernel_forms(pkg, ctx)
    try:
        ctx.set_option(abi.OPT_UNIT_ITEMS, 64)
        ctx.set_option(abi.OPT_PASS_CHUNK, 2)
        for kernel in (abi.KERNEL_ROLL, abi.KERNEL_WAVE):
            if kernel not in forms:
                continue          # (the product library holds the rolling kernel alone; the forms meet in the emulation tier)
            ctx.set_option(abi.OPT_KERNEL, kernel)
            against_oracle(pkg, ctx, oracle, scene, w, h, 9, BOUNCES, tiles, f"ring wrap, kernel form {kernel}")
            assert ("k_pathtrace_roll" in ctx.last_kernel_name()) == (kernel == abi.KERNEL_ROLL), ctx.last_kernel_name()
    finally:
        ctx.set_option(abi.OPT_KERNEL, abi.KERNEL_ROLL)
        ctx.set_option(abi.OPT_UNIT_ITEMS, 2048)
        ctx.set_option(abi.OPT_PASS_CHUNK, 64)


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------------------
def test_step_costs_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the kernel emulation (tests/emu/libcray_hip_emu.so: the render kernels and crh_scene_upload compiled
    unmodified on the HIP-on-CPU shim, where the ring test also renders with the one-unit-at-a-time form) — every one of them runs and passes there, none skipped."""
    run_gpu_tests_on_emulation(__file__, 5)
