"""Variant builds of the kernel emulation (tests/emu/kernel_emu.cpp compiled again with other -D switches) and the child process that renders the fixtures with
one of them: what tests/test_path_record_layout.py and tests/test_record_coop.py share. No test lives here.

Run as a script (`python tests/emu_variants.py NAME ...` with CRH_LIB set) it is that child: it renders each fixture and prints one JSON line per fixture.
"""
import gzip
import hashlib
import json
import os
import subprocess
import sys

from support import EMU_DIR, EMU_LIB, REPO, emulation_env

FIXTURES = ["cfg1_scene", "fence", "refraction", "glowmetal", "nodezoo", "volumes"]
# lanes served by node, shade and retire + refill steps: sums over the paths, so they do not depend on which wave took which job (the rolling kernel's
# step and round counts do: the work queue hands units out in the order the waves ask, which differs from run to run on the emulation as on the GPU)
STEP_KEYS = ("u_node", "u_shade", "u_swap")
# the flags of tests/emu/Makefile's kernel_emu.o
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


def build_variants(out_dir, variants):
    """variants: {tag: [-D switches]} -> the paths of the emulation library built once more per tag (the compiles run side by side), behind the library as the
    Makefile builds it."""
    from conftest import locked_make
    locked_make(["make", "-s", "-C", EMU_DIR, "libcray_hip_emu.so"])
    others = [os.path.join(EMU_DIR, "_obj", o) for o in ("bvh_emu.o", "hipemu.o", "scene_compile.o", "scene_blob.o")]
    built = [(str(out_dir / f"kernel_emu_{tag}.o"), str(out_dir / f"libcray_hip_emu_{tag}.so"), defs) for tag, defs in variants.items()]
    compiles = [subprocess.Popen(["g++"] + EMU_FLAGS + defs + ["-c", os.path.join(EMU_DIR, "kernel_emu.cpp"), "-o", obj]) for obj, _, defs in built]
    assert [c.wait() for c in compiles] == [0] * len(built)
    for obj, lib, _ in built:
        subprocess.check_call(["g++", "-shared", "-pthread", obj] + others + ["-ldl", "-o", lib])
    return (EMU_LIB,) + tuple(lib for _, lib, _ in built)


def render_with_each(libs):
    """The fixtures rendered by one child per library, side by side: per library, the records the children printed."""
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + FIXTURES, env=dict(emulation_env(), CRH_LIB=lib), cwd=REPO,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for lib in libs]
    outs = [p.communicate(timeout=1700)[0] for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-4000:]
    records = [[json.loads(l) for l in out.splitlines() if l.startswith("{")] for out in outs]
    assert all([r["name"] for r in recs] == FIXTURES for recs in records), outs
    return records


if __name__ == "__main__":
    render(sys.argv[1:])
