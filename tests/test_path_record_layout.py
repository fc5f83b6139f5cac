"""CPU tier: the rolling kernel's path table layout (c-ray_amd/csrc/cray_hip.hip: PathTab) changes addresses only.

The lean instantiations of k_pathtrace_roll (no node programs, no volumes) keep a path's words in three arrays — 64-B ray + shading parts,
16-B hit parts, 4-B instance words — instead of one 128-B record per path. The kernel emulation (tests/emu) is built a second time with
-DCRH_PATH_LEAN=0, which restores the 128-B record in every instantiation, and both libraries render the same fixtures: frames, the counters of
counter level 2 and the lanes the scheduler's steps served must be identical, and each frame must equal the reference's float buffer bit for bit.

Fixtures: the lean layout on scenes of many instances (spheres and meshes), with refraction and with emission; node programs and volumes (the
rare-features instantiations, which keep the 128-B record) must come out the same in both builds too. (The instance word has an array of its own
whatever the scene's instance and prim counts, so no scene takes another branch of the layout.)

Run as a script (`python tests/test_path_record_layout.py NAME ...` with CRH_LIB set) it is the child that renders and prints one JSON line per fixture.
"""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(REPO, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libcray_hip_emu.so")
FIXTURES = ["cfg1_scene", "fence", "refraction", "glowmetal", "nodezoo", "volumes"]
# lanes served by node, shade and retire + refill steps: sums over the paths, so they do not depend on which wave took which job (the rolling kernel's
# step and round counts do: the work queue hands units out in the order the waves ask, which differs from run to run on the emulation as on the GPU)
STEP_KEYS = ("u_node", "u_shade", "u_swap")
# the flags of tests/emu/Makefile's kernel_emu.o, plus the layout switch
EMU_FLAGS = ["-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-pthread", "-Wall", "-Wno-attributes", "-Wno-unused-function",
             "-Wno-maybe-uninitialized", "-Wno-unknown-pragmas", "-I" + os.path.join(EMU_DIR, "hipemu"), "-I" + os.path.join(REPO, "include"),
             "-I" + os.path.join(REPO, "c-ray_amd", "csrc"), "-O1", "-DCRH_WITH_ALT_KERNELS", "-DCRH_CENSUS"]


def render(names):
    """Child: render each fixture with the library CRH_LIB names (roll kernel, counter level 2) and print what it computed."""
    import tempfile
    import numpy as np
    sys.path.insert(0, REPO)
    from __graft_entry__ import load_package
    pkg = load_package()
    api, abi = pkg.api, pkg.abi
    golden = os.path.join(REPO, "tests", "golden")
    man = json.load(open(os.path.join(golden, "manifest.json")))
    for name in names:
        m = man[name]
        w, h = m["width"], m["height"]
        with tempfile.NamedTemporaryFile(suffix=".blob") as f:
            f.write(gzip.open(os.path.join(golden, name + ".blob.gz")).read()); f.flush()
            scene = api.Scene(f.name)
        ctx = api.Context(0)
        ctx.set_option(abi.OPT_COUNTER_LEVEL, 2)
        ctx.upload(scene)
        fb = ctx.framebuffer(w, h)
        ctx.reset_counters()
        ctx.render_region(fb, w, h, m["samples"], m["bounces"]); ctx.synchronize()
        img = ctx.download(fb, w, h)
        ticks = ctx.phase_ticks()
        ref_path = os.path.join(golden, name + ".ref.f32.gz")
        ref_equal = None
        if os.path.exists(ref_path):
            ref = np.frombuffer(gzip.open(ref_path).read(), dtype=np.float32)
            ref_equal = bool(np.array_equal(img.ravel().view(np.uint32), ref.view(np.uint32)))
        print(json.dumps({"name": name, "kernel": ctx.last_kernel_name(), "md5": hashlib.md5(img.tobytes()).hexdigest(), "ref_equal": ref_equal,
                          "counters": ctx.counters(), "steps": {k: ticks[k] for k in STEP_KEYS}}), flush=True)
        ctx.close()


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(the emulation library as built, the same source with -DCRH_PATH_LEAN=0)"""
    from conftest import locked_make
    locked_make(["make", "-s", "-C", EMU_DIR, "libcray_hip_emu.so"])
    d = tmp_path_factory.mktemp("lean0")
    obj, lib = str(d / "kernel_emu.o"), str(d / "libcray_hip_emu_lean0.so")
    subprocess.check_call(["g++"] + EMU_FLAGS + ["-DCRH_PATH_LEAN=0", "-c", os.path.join(EMU_DIR, "kernel_emu.cpp"), "-o", obj])
    others = [os.path.join(EMU_DIR, "_obj", o) for o in ("bvh_emu.o", "hipemu.o", "scene_compile.o", "scene_blob.o")]
    subprocess.check_call(["g++", "-shared", "-pthread", obj] + others + ["-ldl", "-o", lib])
    return EMU_LIB, lib


def test_lean_path_table_is_bit_identical_to_the_128_byte_record(libs):
    env = dict(os.environ, CRH_ALLOW_EMULATION="1", HIPEMU_CUS="2", HIPEMU_THREADS="3")
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + FIXTURES, env=dict(env, CRH_LIB=lib), cwd=REPO,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for lib in libs]
    outs = [p.communicate(timeout=1700)[0] for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-4000:]
    lean, wide = ([json.loads(l) for l in out.splitlines() if l.startswith("{")] for out in outs)
    assert [r["name"] for r in lean] == FIXTURES and [r["name"] for r in wide] == FIXTURES, outs
    for a, b in zip(lean, wide):
        assert a["kernel"].startswith("k_pathtrace_roll<2,4,"), a
        assert a == b, (a, b)
        assert a["ref_equal"] in (True, None), a
        assert a["counters"]["rays"] > 0
    # the lean layout was exercised (and the rare-features instantiations were reached too)
    assert any(",false," in r["kernel"] for r in lean) and any(",true," in r["kernel"] for r in lean), [r["kernel"] for r in lean]


if __name__ == "__main__":
    render(sys.argv[1:])
