"""Table N rows a12 / a13 / a14: the nodes no scene JSON reaches — math (15 ops), vecMath (10 ops), fresnel, rayLength,
normal, combineValue, combineRGB, vecToColor, isotropic, nested add — plus the JSON-reachable ones no other fixture uses (add, checker on
a mesh without texture coordinates, blackbody, grayscale(image), NO_BILINEAR fetches).

Fixtures: tests/golden/nodezoo*.{blob,ref.f32}.gz, rendered by the REAL reference with the graphs built by its own C constructors
(oracle/ref_node_patch.c, tools/gen_golden.py). `nodezoo_display` (1 spp, 2 bounces, white background) shows each graph's value as the
colour of one sphere: spheres 0..8 / 18..27 hold the known answers of /root/reference/tests/test_nodes.h as constant graphs (folded by
the scene compiler), 9..17 / 28..37 the same graphs with hit-dependent operands (evaluated per hit by the device VM). `nodezoo` (4 spp,
6 bounces) runs the exotic and JSON graphs through whole paths.

CPU tier: oracle and host-built lane code equal the reference bit for bit. GPU tier: bit for bit as well (c-ray_amd/csrc/exact_math.h);
the Math node's Tangent op included."""
import ctypes as C

import numpy as np
import pytest

from conftest import image_stats
from reference_checks import check_known_answers
from support import emu_render


def test_reference_fixture_shows_the_reference_tests_known_answers(golden_ref):
    """The fixture itself (the real reference's render) reproduces tests/test_nodes.h."""
    check_known_answers(golden_ref("nodezoo_display"))


@pytest.mark.parametrize("name", ["nodezoo_display", "nodezoo"])
def test_oracle_bit_exact_on_node_zoo(name, oracle, manifest, golden_blob, golden_ref):
    m = manifest[name]
    scene = oracle.OracleScene(golden_blob(m["blob"]))
    img, cnt = oracle.render(scene, m["width"], m["height"], m["samples"], m["bounces"])
    ref = golden_ref(name)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{name}: {(img != ref).sum()} floats differ"
    assert cnt["rays"] == m["rays"] and cnt["node_tests"] == m["node_tests"] and cnt["tri_tests"] == m["tri_tests"]


@pytest.mark.parametrize("name", ["nodezoo_display", "nodezoo"])
def test_emulated_kernel_bit_exact_on_node_zoo(name, emu, oracle, manifest, golden_blob, golden_ref):
    """The device lane code + the product's scene compiler (constant folding, operand kinds, postfix programs) built for the host."""
    m = manifest[name]
    scene = oracle.OracleScene(golden_blob(m["blob"]))
    fb, cnt, _ = emu_render(emu, oracle, scene, m["width"], m["height"], m["samples"], m["bounces"])
    ref = golden_ref(name)
    assert np.array_equal(fb.view(np.uint32), ref.view(np.uint32)), f"{name}: {(fb != ref).sum()} floats differ"
    assert cnt["rays"] == m["rays"]


def test_scene_compiler_folds_constant_graphs_and_keeps_dynamic_ones(emu, oracle, golden_blob):
    """Spheres 0..8 / 18..27 are constant graphs: the compiler folds them (no program); 9..17 / 28..37 must stay programs."""
    scene = oracle.OracleScene(golden_blob("nodezoo_display"))
    nprog = C.c_uint32()
    assert emu.emu_compile_check(scene.ptr, None, C.byref(nprog), None) == 0, emu.emu_last_error()
    assert nprog.value >= 19, nprog.value


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nodezoo_display", "nodezoo"])
def test_gpu_node_zoo_vs_reference(name, pkg, manifest, golden_blob, golden_ref):
    if pkg.api.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device; libcray_hip has no CPU fallback")
    m = manifest[name]
    w, h, s, b = m["width"], m["height"], m["samples"], m["bounces"]
    ctx = pkg.api.Context(0)
    try:
        ctx.upload(pkg.api.Scene(golden_blob(m["blob"])))
        fb = ctx.framebuffer(w, h)
        ctx.reset_counters()
        ctx.render_region(fb, w, h, s, b)
        img, cnt = ctx.download(fb, w, h), ctx.counters()
    finally:
        ctx.close()
    ref = golden_ref(name)
    assert cnt["rays"] == m["rays"], (cnt["rays"], m["rays"])
    if name == "nodezoo":
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), image_stats(img, ref)       # every exotic / JSON graph, whole paths: bit-exact
    else:
        check_known_answers(img)
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), image_stats(img, ref)
