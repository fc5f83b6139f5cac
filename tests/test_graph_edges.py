"""Albedo graphs and texture addressing on synthesized scenes: node graphs, textures and texture coordinates that no reference-rendered fixture contains, put
into a copy of nodezoo_display's scene description (tests/scene_synth.py: the geometry and the BVHs stay the fixture's) and probed through the albedo channel of
crh_render_aov — a pure function of the first hit, one pass = evalColor / evalValue / evalImage at every pixel.

The expectation is a restatement (tests/graph_spec.py: Restatement) of the albedo rule (include/cray_hip.h) and of the reference's texture fetch (texture.c:32-79, image.c:31-48, alpha.c,
grayscale.c, color.h) in NumPy float32: recursive, no stack limit, (size_t) wraps as Python integers modulo 2^64, powf from the C library. Its input is the
oracle's hit record of each pixel's camera ray. The CPU tier pins the restatement to the oracle (whose render of a diffuse surface under a white sky IS the
albedo) and, through the reference-rendered fixture `texwrap`, to the reference itself; it also asserts that the synthesized inputs reach the code they are
there for (negative texel indices, the (int) truncation band, wrap at the last texel, x >= 2^32, the grey shortcut's three texel classes) and runs the GPU
tier on the kernel emulation. The GPU tier holds the kernel to the restatement bit for bit, and the frame of the same descriptions to the oracle's.

Out of scope, because the reference itself is undefined C there: a nearest fetch at a negative uv ((size_t) of a negative float) and a
filtered fetch with |uv * size| >= 2^31 ((int) of a float out of range). The inputs avoid both and the restatement asserts that they do; the float texels are
not negative, so no NaN arises (every expectation is asserted finite).

The reference's loaders give 8-bit textures of 3 or 4 channels (and float RGB from .hdr files) only, so the 1-channel and the float RGBA textures, and every
graph built here, stay with the oracle and the restatement; the 7 x 6 RGBA and 16 x 16 RGB 8-bit textures are also held to the reference by `texwrap`."""
import re

import numpy as np
import pytest

from conftest import resize_camera
from firsthit_spec import fold
from graph_spec import (CUBE, MESH_CAMERA_A, MESH_H, MESH_W, NB, PLANE, SPHERES_H, SPHERES_W, F, ForLibrary, Restatement, S, assert_aov, base, gpu_aov, scene_hits, size_of,  # noqa: F401
                        white_sky_selection)          # (base: the module-scoped fixture of nodezoo_display's scene)
from scene_synth import ADD, DIFFUSE, EMISSION, GLASS, ISOTROPIC, METAL, MIX, NONE, PLASTIC, TRANSPARENT, SynthScene
from support import DeviceArray, ctx, run_gpu_tests_on_emulation  # noqa: F401 (ctx: the fixture)

ADD_DEPTH = 4          # CRH_ADD_DEPTH (c-ray_amd/csrc/pt_device.h)
AOV_DEPTH = 8          # CRH_AOV_ALBEDO_DEPTH (include/cray_hip.h)


def mix_depth(desc, j):
    """Open mix / add frames under bsdf node j (CompiledScene::max_albedo_depth)."""
    n = desc.gnodes[j]
    if n.kind in (MIX, ADD):
        return 1 + max(mix_depth(desc, n.a), mix_depth(desc, n.b))
    return mix_depth(desc, n.c) if n.kind == PLASTIC else 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The synthesized scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def make_textures():
    """name -> pixels in stored row order; fixed seed; 8-bit ones hold 0 and 255."""
    rng = np.random.default_rng(20261017)

    def u8(h, w, ch):
        a = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        a.reshape(-1)[0], a.reshape(-1)[-1] = 0, 255
        return a
    t = {"rgb1x1": np.array([[[255, 0, 77]]], np.uint8),
         "rgbaf2x2": rng.random((2, 2, 4), dtype=F),
         "rgba7x6": u8(6, 7, 4),
         "l13x1": u8(1, 13, 1),
         "lf1x9": rng.random((9, 1, 1), dtype=F),
         "rgbf8x4": rng.random((4, 8, 3), dtype=F) * F(4.0)}
    # for the sRGB transform's grey shortcut: columns 0..4 grey, 5..9 r = g != b, the rest free (in blocks, so that a filtered fetch stays inside a class)
    s = u8(16, 16, 3).reshape(-1, 3)
    col = np.arange(256) % 16
    grey, two, free = col < 5, (col >= 5) & (col < 10), col >= 10
    s[grey, 1] = s[grey, 0]
    s[grey, 2] = s[grey, 0]
    s[two, 1] = s[two, 0]
    s[two, 2] = np.where(s[two, 2] == s[two, 0], s[two, 0] ^ 0x55, s[two, 2])
    s[free, 1] = np.where(s[free, 1] == s[free, 0], s[free, 0] ^ 0x33, s[free, 1])
    s[255] = 255
    t["srgb16"] = s.reshape(16, 16, 3)
    return t


TEXTURES = make_textures()
TEX_NAMES = list(TEXTURES)
# every texture filtered and nearest; the 7 x 6 and the 16 x 16 ones with and without the sRGB transform
IMAGE_CONFIGS = [(n, o) for n in TEX_NAMES for o in (0, NB)] + [(n, o) for n in ("rgba7x6", "srgb16") for o in (S, S | NB)]
FILTERED = [c for c in IMAGE_CONFIGS if not c[1] & NB]


def texcoord_map(variant, name):
    """uv' = scale * uv + offset of the plane's texture coordinates, per axis."""
    h, w = TEXTURES[name].shape[0:2]
    return {"identity": ((1.0, 1.0), (0.0, 0.0)),
            "tiling": ((5.3, 5.3), (-2.6, -2.6)),                                  # tiles, and negative
            "band": ((3.0 / w, 3.0 / h), (-1.5 / w, -1.5 / h)),                    # uv * size - 0.5 spans (-2, 1): the band where (int) truncates towards zero
            "far": ((1e5, 1e5), (0.0, 0.0)),
            "veryfar": ((2e9, 2e9), (0.0, 0.0))}[variant]                         # nearest only: x >= 2^32


# (variant, (texture, options)) of the textured plane: one scene each
MESH_PAIRS = ([("identity", c) for c in IMAGE_CONFIGS] + [(v, c) for v in ("tiling", "band", "far") for c in FILTERED]
              + [("veryfar", c) for c in (("rgba7x6", NB), ("l13x1", NB), ("rgba7x6", S | NB))])


def chain(s, ops, right, leaves, factors):
    """A chain of mix / add nodes, ops[0] at the root: right-deep op(leaf_k, next) — every level's a colour waits while the b branch is evaluated —
    or left-deep op(next, leaf_k) — every level's node word waits. len(leaves) == len(ops) + 1; factors[k] is level k's (ignored by add)."""
    node = leaves[len(ops)]
    for k in reversed(range(len(ops))):
        a, b = (leaves[k], node) if right else (node, leaves[k])
        node = s.bsdf(ops[k], a, b, factors[k] if ops[k] == MIX else NONE)
    return node


def build_scene(base, plane=("rgba7x6", S), variant="identity", view="spheres", extra=None):
    """Every sphere of nodezoo gets a graph of its own, the cube a filtered image (it has no texture coordinates: uv = (-1, -1)), the plane diffuse(image `plane`)
    with its texture coordinates mapped by `variant`. Returns the scene and label -> material."""
    s = SynthScene(base)
    s.drop_textures()
    tex = {n: s.texture(p) for n, p in TEXTURES.items()}
    assert len(tex) >= base.desc.texture_count          # (the fixture's own image nodes keep valid texture indices; no object shows them)
    labels = {}

    def img(name, options=0):
        return s.image(tex[name], options)

    def D(c):
        return s.bsdf(DIFFUSE, c)

    count = [0]

    def leaf():          # diffuse leaves of distinct colours
        k = count[0] = count[0] + 1
        return D(s.color(0.03 + 0.011 * k, 0.97 - 0.009 * k, 0.1 + 0.031 * (k % 29)))

    def add(label, bsdf, ior=1.45):
        assert label not in labels
        labels[label] = s.material(bsdf, ior=ior)

    for name, o in IMAGE_CONFIGS:
        add(f"diffuse({name},{o})", D(img(name, o)))
    add("metal(image)", s.bsdf(METAL, img("rgbf8x4"), s.value(0.2)))
    add("glass(image)", s.bsdf(GLASS, img("srgb16", S), s.value(0.05), s.value(1.5)))
    add("transparent(image)", s.bsdf(TRANSPARENT, img("rgbaf2x2", NB)))
    add("isotropic(image)", s.bsdf(ISOTROPIC, img("l13x1")))
    add("image without texture", D(s.image(NONE, 0)))
    add("emission * 2.5", s.bsdf(EMISSION, img("rgba7x6", NB), s.value(2.5)))
    add("emission * grayscale(image)", s.bsdf(EMISSION, s.color(0.9, 0.5, 0.2), s.grayscale(img("srgb16"))))
    add("emission * alpha(image)", s.bsdf(EMISSION, img("rgbf8x4"), s.alpha(img("rgba7x6"))))
    add("plastic over diffuse(image)", s.bsdf(PLASTIC, s.color(1.0, 1.0, 1.0), s.color(0.1, 0.1, 0.1), D(img("lf1x9"))))
    add("plastic over mix", s.bsdf(PLASTIC, s.color(1.0, 1.0, 1.0), s.color(0.1, 0.1, 0.1), s.bsdf(MIX, leaf(), D(img("rgba7x6", S)), s.value(0.3))))
    for v in (0.0, 1.0, 0.25, 1.5, -0.5):          # cmix does not clamp
        add(f"mix {v}", s.bsdf(MIX, leaf(), D(img("rgbaf2x2")), s.value(v)))
    add("mix alpha(image)", s.bsdf(MIX, leaf(), D(img("srgb16", NB)), s.alpha(img("rgba7x6"))))
    add("mix grayscale(image)", s.bsdf(MIX, D(img("rgbf8x4", NB)), leaf(), s.grayscale(img("rgba7x6", S))))

    def chain_of(ops, right):
        n = len(ops)
        leaves = [leaf() for _ in range(n)] + [D(img("rgba7x6"))]
        factors = [s.value(0.07 + 0.11 * k) for k in range(n)]
        factors[n - 1] = s.alpha(img("rgba7x6", NB))          # the deepest level's factor depends on the hit
        if n > 2:
            factors[1] = s.grayscale(img("srgb16"))
        return chain(s, ops, right, leaves, factors)

    for depth in (1, 2, 3, 4, 5, 6, 7, 8):
        for right in (False, True):
            add(f"mix chain {depth} {'right' if right else 'left'}", chain_of([MIX] * depth, right))
    for right in (False, True):
        add(f"add chain {ADD_DEPTH} {'right' if right else 'left'}", chain_of([ADD] * ADD_DEPTH, right))
    add("mix / add alternating 8", chain_of([MIX, ADD] * 4, True))
    add("add / mix alternating 8 left", chain_of([ADD, MIX] * 4, False))

    def tree(depth):
        if depth == 0:
            return leaf() if count[0] % 3 else D(img("rgbaf2x2"))
        return s.bsdf(MIX, tree(depth - 1), tree(depth - 1), s.alpha(img("rgba7x6")) if depth == 1 else s.value(0.2 * depth))
    add("balanced mix tree 3", tree(3))
    if extra:
        for label, ops, right in extra:
            add(label, chain_of(ops, right))
    names = list(labels)
    assert len(names) <= 60 == base.desc.sphere_count          # every graph has a sphere of its own, and every sphere a graph
    for i in range(60):
        s.set_sphere_material(i, labels[names[i % len(names)]])
    labels["cube"] = s.material(D(img("rgba7x6")))
    s.set_mesh_material(CUBE, labels["cube"])
    labels["plane"] = s.material(D(img(*plane)))
    s.set_mesh_material(PLANE, labels["plane"])
    scale, offset = texcoord_map(variant, plane[0])
    s.map_texcoords(PLANE, scale, offset)
    cam = s.desc.camera
    if view == "mesh":
        for k in range(12):
            cam.A[k] = MESH_CAMERA_A[k]
        resize_camera(s, MESH_W, MESH_H)
    else:
        resize_camera(s, SPHERES_W, SPHERES_H)
    return s, labels


_cases = {}


def cpu_case(oracle, base, variant, config):
    """One scene of the textured plane: (scene, labels, pass-0 hits, restatement with its probes, expected albedo) — computed once, shared, left unchanged."""
    key = (variant, config)
    if key not in _cases:
        view = "spheres" if variant == "spheres" else "mesh"
        s, labels = build_scene(base, view=view) if variant == "spheres" else build_scene(base, plane=config, variant=variant, view=view)
        hits = scene_hits(oracle, s, view)[0]
        r = Restatement(s.desc)
        want = r.frame(hits)
        assert np.isfinite(want).all()
        _cases[key] = (s, labels, hits, r, want)
    return _cases[key]


GROUPS = {"spheres": [("spheres", None)]}
for _v, _c in MESH_PAIRS:
    GROUPS.setdefault(_v, []).append((_v, _c))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def plane_probe(case):
    """The image fetch of the plane's pixels: its probe, restricted to nothing else (the plane's material is evaluated on its own pixels)."""
    s, labels, hits, r, _ = case
    sel = (hits["inst"] >= 0) & (hits["material"] == labels["plane"])
    rr = Restatement(s.desc)
    rr.albedo(s.desc.materials[labels["plane"]].bsdf, hits[sel])
    assert len(rr.probes) == 1
    return rr.probes[0], int(sel.sum())


def classes_of(p):
    """How many of a fetch's pixels fall into each class of the texture-addressing code."""
    c = {}
    W, H = p["width"], p["height"]
    if "xint" in p:
        for a, n, size in (("x", "xint", W), ("y", "yint", H)):
            i, f = p[n], p["f" + a]
            c[a + "neg"] = int((i < 0).sum())                          # a negative index: wrapIndex's (size_t) branch
            c[a + "0neg"] = int(((i == 0) & (f < 0)).sum())            # (int) truncated towards zero: index 0 with a negative blend factor
            c[a + "wrap"] = int(((p["t" + a] == size - 1) & (p["t" + a + "1"] == 0)).sum())          # the last texel, and the second one wraps to 0
    else:
        c["xbig"] = int((p["x"] >= 2.0 ** 32).sum())
        c["ybig"] = int((p["y"] >= 2.0 ** 32).sum())
    if "fetched" in p and W == 16:
        b = p["fetched"].view(np.uint32)
        grey = (b[:, 0] == b[:, 1]) & (b[:, 1] == b[:, 2])
        two = (b[:, 0] == b[:, 1]) & ~grey
        c["grey"], c["two"], c["free"] = int(grey.sum()), int(two.sum()), int((~grey & ~two).sum())
    return c


def required_classes(variant, config):
    """The classes a (variant, texture) pair CAN reach: each must show at least 50 pixels."""
    name, o = config
    h, w = TEXTURES[name].shape[0:2]
    if o & NB:
        need = [a + "big" for a, size in (("x", w), ("y", h)) if size * 2e9 >= 2.0 ** 32] if variant == "veryfar" else []
    else:
        need = {"identity": ["x0neg", "xwrap", "y0neg", "ywrap"],
                "tiling": ["xneg", "x0neg", "xwrap", "yneg", "y0neg", "ywrap"],
                "band": ["xneg", "x0neg", "yneg", "y0neg"] + (["xwrap"] if w == 1 else []) + (["ywrap"] if h == 1 else []),          # indices -1 and 0 only
                "far": ["xwrap", "ywrap"]}[variant]
    if o & S and name == "srgb16" and variant != "band":          # (the band is columns 14, 15, 0 and 1)
        need = need + ["grey", "two", "free"]
    return need


@pytest.mark.parametrize("variant", [g for g in GROUPS if g != "spheres"])
def test_inputs_reach_the_addressing_classes(variant, oracle, base):
    """f. Conditions, not measurements: every texture x variant pair shows at least 50 pixels in each class it can reach."""
    for _, config in GROUPS[variant]:
        probe, pixels = plane_probe(cpu_case(oracle, base, variant, config))
        got = classes_of(probe)
        need = required_classes(variant, config)
        print(f"{variant} {config[0]} options {config[1]}: {pixels} pixels, {got}")
        assert pixels >= 2000
        for c in need:
            assert got[c] >= 50, (variant, config, c, got)


def test_inputs_reach_every_graph_and_the_mesh_without_texcoords(oracle, base):
    """f. Every graph's sphere shows at least 30 hit pixels; the cube's filtered fetch at uv = (-1, -1) has negative indices; the deepest chains are as deep as the evaluator allows."""
    s, labels, hits, r, _ = cpu_case(oracle, base, "spheres", None)
    hit = hits["inst"] >= 0
    counts = {label: int((hit & (hits["material"] == m)).sum()) for label, m in labels.items()}
    print(counts)
    low = {k: v for k, v in counts.items() if v < 30}
    assert not low, low
    d = s.desc
    depths = {label: mix_depth(d, d.materials[m].bsdf) for label, m in labels.items()}
    assert max(depths.values()) == AOV_DEPTH and depths["mix chain 8 right"] == 8 and depths["mix chain 8 left"] == 8 and depths["mix / add alternating 8"] == 8
    sel = hit & (hits["material"] == labels["cube"])
    rr = Restatement(d)
    rr.albedo(d.materials[labels["cube"]].bsdf, hits[sel])
    assert (hits["uv"][sel] == F(-1.0)).all()
    c = classes_of(rr.probes[0])
    print("cube", c)
    assert c["xneg"] >= 50 and c["yneg"] >= 50


@pytest.mark.parametrize("variant", [g for g in GROUPS if g != "spheres"])
def test_restatement_equals_the_oracles_render_under_a_white_sky(variant, oracle, base):
    """g. The restatement pinned to the oracle on every texture x variant pair (the plane's material is diffuse(image))."""
    for _, config in GROUPS[variant]:
        _, labels, hits, _, want = cpu_case(oracle, base, variant, config)
        s, _ = build_scene(base, plane=config, variant=variant, view="mesh")          # (a copy of its own: the shared case keeps its sky)
        img, sel = white_sky_selection(oracle, s, hits, "mesh")
        plane = (hits["inst"] >= 0) & (hits["material"] == labels["plane"])
        chosen = sel & plane
        print(f"{variant} {config}: {int(chosen.sum())} of {int(plane.sum())} plane pixels")
        assert 2 * chosen.sum() >= plane.sum()
        assert np.array_equal(img[sel].view(np.uint32), want[sel].view(np.uint32)), (variant, config, int((img[sel] != want[sel]).any(axis=1).sum()))


def test_restatement_equals_the_oracles_render_on_the_spheres(oracle, base):
    """g. ... and on the spheres whose root is diffuse (every image configuration on a sphere's own uv, the missing texture) and on the cube."""
    _, labels, hits, _, want = cpu_case(oracle, base, "spheres", None)
    s, _ = build_scene(base, view="spheres")
    img, sel = white_sky_selection(oracle, s, hits, "spheres")
    hit = hits["inst"] >= 0
    for label, m in labels.items():
        if label.startswith("diffuse(") or label in ("cube", "image without texture"):
            here = hit & (hits["material"] == m)
            assert 2 * (sel & here).sum() >= here.sum(), label
    assert np.array_equal(img[sel].view(np.uint32), want[sel].view(np.uint32)), int((img[sel] != want[sel]).any(axis=1).sum())


def test_restatement_equals_the_references_render_of_texwrap(oracle, manifest, golden_blob, golden_ref):
    """The fixture `texwrap` (tools/gen_golden.py: the real reference's render of eight quads whose OBJ texture coordinates carry the identity, tiling / negative,
    band and far ranges, on a 7 x 6 RGBA and a 16 x 16 RGB 8-bit PNG, under a constant white sky) pins the restatement, and the oracle, to the reference:
    where a quad's root is diffuse(image) or emission(colour, grayscale(image)) and the second ray escaped, the reference's pixel of the 1-sample, 2-bounce
    frame IS the albedo. What the reference's
    loaders cannot produce stays with the oracle and the restatement alone: 1-channel textures, float textures with alpha, textures of one texel's width,
    coordinates with x >= 2^32 on a nearest fetch (an OBJ holds them, but the frame would need 2e9 as a float in the file: kept synthetic), the missing
    texture, and every bsdf graph but diffuse, emission and mix(.., .., grayscale(image)) — the latter is in the full-path frame of `texwrap` that
    tests/test_oracle_golden.py holds the oracle to."""
    m = manifest["texwrap_display"]
    w, h = m["width"], m["height"]
    assert (w, h) == size_of("texwrap") and m["samples"] == 1 and m["blob"] == "texwrap"
    scene = oracle.OracleScene(golden_blob("texwrap"))
    ref = golden_ref("texwrap_display")
    img = oracle.render(scene, w, h, 1, m["bounces"], threads=1)[0]
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"the oracle: {int((img != ref).sum())} floats differ"
    hits = scene_hits(oracle, scene, "texwrap")[0]
    d = scene.desc
    r = Restatement(d)
    want = r.frame(hits)
    hit = hits["inst"] >= 0
    escaped = (ref != 0).any(axis=2)
    checked, classes = 0, {}
    for mat in np.unique(hits["material"][hit]):
        here = hit & (hits["material"] == mat)
        if d.gnodes[d.materials[int(mat)].bsdf].kind not in (DIFFUSE, EMISSION):          # (an emission node scatters like a diffuse one, attenuated by colour x strength)
            continue
        sel = here & escaped
        assert 2 * sel.sum() >= here.sum() >= 500, (int(mat), int(sel.sum()), int(here.sum()))
        assert np.array_equal(ref[sel].view(np.uint32), want[sel].view(np.uint32)), f"material {mat}: {int((ref[sel] != want[sel]).any(axis=1).sum())} pixels differ"
        checked += 1
        rr = Restatement(d)
        rr.albedo(d.materials[int(mat)].bsdf, hits[here])
        for k, v in classes_of(rr.probes[0]).items():
            classes[k] = max(classes.get(k, 0), v)
    print(f"{checked} diffuse and emission quads; most pixels of one quad per class: {classes}")
    assert checked == 9
    for c in ("xneg", "x0neg", "xwrap", "yneg", "y0neg", "ywrap", "grey", "two", "free"):
        assert classes[c] >= 50, (c, classes)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_albedo_equals_the_restatement(group, pkg, ctx, oracle, base):
    """a. One pass of one on every variant: every hit pixel's albedo, a miss's eight zeros, the geometry channels."""
    for variant, config in GROUPS[group]:
        s, _, hits, _, want = cpu_case(oracle, base, variant, config)
        w, h = size_of("spheres" if variant == "spheres" else "mesh")
        got = gpu_aov(pkg, ctx, s, w, h, 1)
        assert (hits["inst"] >= 0).sum() >= 2000
        assert_aov(got, want, hits[None], [0], f"{variant} {config}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant,config", [("spheres", None), ("tiling", ("rgba7x6", S))])
def test_albedo_of_three_passes_folds_like_the_frame(variant, config, pkg, ctx, oracle, base):
    """b. Three passes of three: the restatement per pass, folded with the running mean."""
    view = "spheres" if variant == "spheres" else "mesh"
    s = cpu_case(oracle, base, variant, config)[0]
    w, h = size_of(view)
    hits = scene_hits(oracle, s, view, passes=range(3), max_passes=3)
    r = Restatement(s.desc)
    want = np.zeros((h, w, 3), F)
    for p in range(3):
        want = fold(want, r.frame(hits[p]), p + 1)
    got = gpu_aov(pkg, ctx, s, w, h, 3)
    assert_aov(got, want, hits, range(3), f"{variant} {config}")


RENDER_CASES = [("tiling", ("rgba7x6", S), False), ("tiling", ("rgba7x6", S), True), ("far", ("srgb16", S), False), ("spheres", None, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,config,halton", RENDER_CASES, ids=[f"{v}-{'halton' if hl else 'random'}" for v, _, hl in RENDER_CASES])
def test_frame_equals_the_oracles(variant, config, halton, pkg, ctx, oracle, base):
    """c. crh_render_region at 4 samples and 6 bounces against oracle.render of the same description: the frame bit for bit, and the ray count."""
    s = cpu_case(oracle, base, variant, config)[0]
    w, h = size_of("spheres" if variant == "spheres" else "mesh")
    want, ocnt = oracle.render(s, w, h, 4, 6, halton=halton, threads=1 if halton else 0)
    ctx.set_option(pkg.abi.OPT_SAMPLER, pkg.abi.SAMPLER_HALTON if halton else pkg.abi.SAMPLER_RANDOM)
    try:
        ctx.upload(ForLibrary(pkg, s))
        fb = ctx.framebuffer(w, h)
        ctx.reset_counters()
        ctx.render_region(fb, w, h, 4, 6)
        got = ctx.download(fb, w, h)
        rays = ctx.counters()["rays"]
    finally:
        ctx.set_option(pkg.abi.OPT_SAMPLER, pkg.abi.SAMPLER_RANDOM)
    assert want.any() and np.isfinite(want).all()
    assert rays == ocnt["rays"]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} floats differ"


@pytest.mark.gpu
def test_a_graph_nested_nine_deep_renders_but_has_no_albedo(pkg, ctx, oracle, base):
    """d. A mix chain of depth 9: the frame is the oracle's; crh_render_aov answers CRH_ERR_UNSUPPORTED with the depth in its message and touches nothing;
    the depth-8 scene on the same context has its albedo again."""
    api, abi = pkg.api, pkg.abi
    w, h = SPHERES_W, SPHERES_H
    deep, labels = build_scene(base, view="spheres", extra=[("mix chain 9 right", [MIX] * 9, True)])
    assert mix_depth(deep.desc, deep.desc.materials[labels["mix chain 9 right"]].bsdf) == AOV_DEPTH + 1
    hits = scene_hits(oracle, deep, "spheres")[0]
    assert ((hits["inst"] >= 0) & (hits["material"] == labels["mix chain 9 right"])).sum() >= 30
    ctx.upload(ForLibrary(pkg, deep))
    fb = ctx.framebuffer(w, h)
    ctx.reset_counters()
    ctx.render_region(fb, w, h, 4, 6)
    got = ctx.download(fb, w, h)
    want, ocnt = oracle.render(deep, w, h, 4, 6)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    before = (ctx.counters(), ctx.kernel_time_ms(), ctx.last_kernel_name())
    assert before[0]["rays"] == ocnt["rays"]
    sentinel = np.arange(w * h * 8, dtype=F).reshape(h, w, 8) + F(0.5)
    dev = DeviceArray(pkg, sentinel)
    with pytest.raises(api.CrhError) as e:
        ctx.render_aov(dev.ptr, w, h, 1)
    assert e.value.code == abi.ERR_UNSUPPORTED
    assert re.search(r"\b9\b", str(e.value)), str(e.value)
    assert np.array_equal(dev.read(ctx), sentinel), "a refused dispatch wrote into the buffer"
    assert (ctx.counters(), ctx.kernel_time_ms(), ctx.last_kernel_name()) == before
    s, _, hits, _, want = cpu_case(oracle, base, "spheres", None)
    assert_aov(gpu_aov(pkg, ctx, s, w, h, 1), want, hits[None], [0], "the depth-8 scene after the refused one")


@pytest.mark.gpu
def test_add_nodes_nested_too_deep_are_refused_at_upload(pkg, ctx, oracle, base):
    """e. An add chain of depth CRH_ADD_DEPTH + 1: crh_scene_upload answers CRH_ERR_UNSUPPORTED, and the context still works."""
    bad, _ = build_scene(base, view="spheres", extra=[("add chain 5", [ADD] * (ADD_DEPTH + 1), True)])
    with pytest.raises(pkg.api.CrhError) as e:
        ctx.upload(ForLibrary(pkg, bad))
    assert e.value.code == pkg.abi.ERR_UNSUPPORTED, str(e.value)
    s, _, hits, _, want = cpu_case(oracle, base, "spheres", None)
    assert_aov(gpu_aov(pkg, ctx, s, SPHERES_W, SPHERES_H, 1), want, hits[None], [0], "after the refused upload")


def test_graph_edges_on_the_emulation():
    """h. CPU tier: this file's GPU tests run by a child pytest against the kernel emulation (tests/emu/libcray_hip_emu.so: k_aov, the render kernels and the
    scene compiler compiled unmodified on the HIP-on-CPU shim) — every one of them runs and passes there, none skipped."""
    run_gpu_tests_on_emulation(__file__, len(GROUPS) + 2 + len(RENDER_CASES) + 2)
