"""What the test files share and none of them owns (a plain helper module like scene_synth.py, not a conftest): the device-context fixture, caller-owned device
buffers, bit comparisons, the drop-in program's child runs, the child pytest that runs a file's GPU tests on the kernel emulation, the lane emulation's render call
and the one-line C program that reads include/cray_hip.h. No test module imports another: what two of them need lives here or in a module named for its subject
(denoise_spec, adaptive_spec, firsthit_spec, exr_reader, graph_spec, reference_checks, emu_variants)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(REPO, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libcray_hip_emu.so")
DROPIN_LIBDIR = os.path.join(EMU_DIR, "_dropin_libs")          # (tests/emu/Makefile: the emulation library under the product library's name)
f32 = np.float32


@pytest.fixture(scope="module")
def ctx(pkg):
    """A device context per test module: `from support import ctx` (a fixture imported into a module's namespace keeps its module scope there)."""
    if pkg.api.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device; libcray_hip has no CPU fallback")
    c = pkg.api.Context(0)
    yield c
    c.close()


class DeviceArray:
    """A caller-owned device buffer filled by the caller (the entry points take any device pointer): a torch tensor on the GPU; under the kernel emulation, whose
    device memory is the host heap, a numpy array. dtype None keeps the values' own; uint32 words travel as int32 bits (torch's everyday dtype)."""

    def __init__(self, pkg, values, dtype=np.float32):
        values = np.ascontiguousarray(values, dtype)
        self.dtype = values.dtype
        self.emulated = hasattr(pkg.api.library(), "crh_emu_stats")
        if self.emulated:
            self.a = values.copy()
            self.ptr = self.a.ctypes.data
        else:
            import torch
            self.a = torch.from_numpy(values.view(np.int32 if values.dtype == np.uint32 else values.dtype).copy()).to("cuda:0")
            torch.cuda.synchronize()
            self.ptr = self.a.data_ptr()
        assert self.ptr % 16 == 0

    def read(self, ctx):
        ctx.synchronize()
        return self.a.copy() if self.emulated else self.a.cpu().numpy().view(self.dtype)


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what):
    """got holds want's bits, NaNs and infinities included; prints and reports how many floats differ and where the first one is."""
    assert got.shape == want.shape, f"{what}: shape {got.shape}, want {want.shape}"
    bad = np.flatnonzero(bits(got) != bits(want))
    print(f"{what}: {bad.size} of {want.size} floats differ")
    assert bad.size == 0, f"{what}: {bad.size} floats differ, the first at index {bad[0]}"


def assert_bit_equal(got, want, what):
    """same_bits, and every float is finite."""
    same_bits(got, want, what)
    assert np.isfinite(got).all(), what


# ---- the drop-in program ------------------------------------------------------------------------------------------------------------------
def dropin_paths():
    """(c-ray-hip, the asset overlay it runs in, whether both are built)"""
    exe = os.path.join(REPO, "c-ray_amd", "_lib", "c-ray-hip")
    overlay = os.path.join(REPO, "oracle", "_ref", "input")
    return exe, overlay, os.path.exists(exe) and os.path.exists(os.path.join(overlay, "scene.json"))


def dropin_env():
    """Extra environment of the c-ray-hip child processes. Empty on a GPU box. The CPU tier runs these tests against the kernel emulation: CRH_DROPIN_LIBDIR
    names a directory whose libcray_hip.so IS the emulation library, and the program's loader finds it there before its RUNPATH."""
    libdir = os.environ.get("CRH_DROPIN_LIBDIR")
    return {"LD_LIBRARY_PATH": libdir + ":" + os.environ.get("LD_LIBRARY_PATH", "")} if libdir else {}


def run_dropin(manifest, out_dir, env, tile=None):
    """c-ray-hip on cfg1_scene, its files in out_dir: one device, no feature variable inherited from the caller's environment, then `env` (which names the features
    and the dumps a test asks for). Returns {file name: bytes} of everything in out_dir and the program's output."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import refrun
    exe, overlay, _ = dropin_paths()
    m = manifest["cfg1_scene"]
    os.makedirs(out_dir, exist_ok=True)
    scene = refrun.rewrite_scene("scene.json", m["width"], m["height"], m["samples"], m["bounces"], tile=tile, out_dir=str(out_dir))
    child = {k: v for k, v in os.environ.items() if not k.startswith("CRAY_HIP_") and k not in ("CRH_DENOISE_FORM", "CRH_DROPIN_PASSES")}
    child["CRAY_HIP_DEVICES"] = "1"
    child.update(env)
    proc = subprocess.run([exe], input=json.dumps(scene).encode(), cwd=overlay, env=child, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = proc.stdout.decode(errors="replace")
    assert proc.returncode == 0, text[-2000:]
    return {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}, text


# ---- the CPU tier's emulations ------------------------------------------------------------------------------------------------------------
def emulation_env(**more):
    """The environment of a child process whose api.py binds to the kernel emulation: two compute units on three OS threads."""
    return dict(os.environ, CRH_LIB=EMU_LIB, CRH_ALLOW_EMULATION="1", HIPEMU_CUS="2", HIPEMU_THREADS="3", **more)


def emulated_dropin(*libs):
    """Whether the drop-in tests can run on the emulation: the program and its overlay are built, and so is the directory the program loads the emulation from
    (with `libs` in it)."""
    return bool(dropin_paths()[2]) and os.path.isdir(DROPIN_LIBDIR) and all(os.path.exists(os.path.join(DROPIN_LIBDIR, lib)) for lib in libs)


def run_gpu_tests_on_emulation(test_file, passed, passed_without_dropin=None, extra_env=None, make_targets=("libcray_hip_emu.so",), show_output=False, dropin_libs=(),
                               timeout=1700):
    """The CPU tier of a test file: its GPU tests run by a child pytest against the kernel emulation (tests/emu: the kernels and their entry points compiled
    unmodified on the HIP-on-CPU shim). Exactly `passed` of them pass and none is skipped; a file with drop-in tests says how many pass where the drop-in program
    is not built (`passed_without_dropin`: those tests are deselected there). Every entry of make_targets is one make in tests/emu. Returns the child's output."""
    from conftest import locked_make
    for target in make_targets:
        locked_make(["make", "-s", "-C", EMU_DIR] + target.split())
    env, select = emulation_env(**(extra_env or {})), []
    if passed_without_dropin is not None:
        env["CRH_DROPIN_LIBDIR"] = DROPIN_LIBDIR
        if not emulated_dropin(*dropin_libs):
            passed, select = passed_without_dropin, ["-k", "not dropin"]
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(test_file), "-m", "gpu", "-q", "-x"] + (["-s"] if show_output else []) + ["-p", "no:cacheprovider"] + select
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=timeout)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == passed, tail
    assert "skipped" not in r.stdout.strip().splitlines()[-1], tail
    return r.stdout


def emu_render(emu, oracle, scene, w, h, s, b, region=None, shape=(8, 8), chunk=64):
    """The lane emulation (conftest's `emu`: tests/emu/libcray_emu.so) renders a region: the frame, the counters, the traversal stack's high-water mark."""
    abi = oracle.abi
    x0, y0, x1, y1 = region or (0, 0, w, h)
    fb = np.zeros((h, w, 3), np.float32)
    cnt, hi = abi.Counters(), C.c_uint32()
    p = abi.RenderParams(x0, y0, x1, y1, w, h, 0, s, s, b)
    rc = emu.emu_render_region(scene.ptr, C.byref(p), fb.ctypes.data, C.byref(cnt), C.byref(hi), shape[0], shape[1], chunk)
    assert rc == 0, emu.emu_last_error()
    return fb, cnt.as_dict(), hi.value


# ---- the header --------------------------------------------------------------------------------------------------------------------------
def header_values(tmp_path, *c_expressions):
    """The values of integer expressions of C — sizeof(a struct), offsetof, a constant — as include/cray_hip.h defines them: a one-line program, compiled and run."""
    src, exe = tmp_path / "header_values.c", tmp_path / "header_values"
    prints = "".join(f'printf("%lld\\n", (long long)({e}));' for e in c_expressions)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cray_hip.h"\nint main(void){' + prints + "return 0;}\n")
    subprocess.check_call(["gcc", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    return [int(v) for v in subprocess.check_output([str(exe)]).split()]
