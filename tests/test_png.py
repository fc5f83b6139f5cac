"""The 8-bit frame as a PNG file, filtered, deflated and check-summed on the device: crx_png_pack of the companion library libcray_hip_exr.so
(include/cray_hip_exr.h, c-ray_amd/csrc/png_pack.h), ZipContext.png and Context.write_png around it, CRAY_HIP_PNG=1 of the drop-in program.

The reader is independent of the code under test: a chunk walker (signature, order, lengths, every CRC by zlib.crc32), zlib.decompress of the IDAT (which verifies
the Adler-32), PIL for the pixels, and a NumPy restatement of the five filters and of the min-sum rule for the filtered bytes and the chosen types. CPU tier: the
restatement anchored to PIL, and this file's GPU tests run by a child pytest on the emulation. GPU tier: shapes whose n = (3 W + 1) H is word-unaligned and whose
segments end mid-row, crafted rows for every filter type, values at the conversion's edges, a rendered frame with tEXt chunks, the CRC alone, determinism and sizes,
refusals, the drop-in program."""
import ctypes as C
import io
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

from support import EMU_DIR, REPO, DeviceArray, ctx, dropin_env, dropin_paths, run_gpu_tests_on_emulation  # noqa: F401 (ctx: the fixture)

SIGNATURE = b"\x89PNG\r\n\x1a\n"
FILTERS = ("adaptive", "none", "sub", "up", "average", "paeth")          # "adaptive", then the types 0 .. 4
SEG = 4096          # (asserted against crx_zip_segment_bytes where it matters)
SMALL = [(1, 1), (2, 1), (3, 1), (2, 3)]          # n mod 4 = 0, 3, 2, 1
SHAPES = SMALL + [(341, 4), (80, 17), (341, 8), (500, 9), (400, 880)]          # n = 4096; 4097; two whole segments; rows across segment ends; 259 segments


# ---- the reader ---------------------------------------------------------------------------------------------------------------------------
def walk(data):
    """[(type, payload)] of a PNG file: the signature, every chunk's length and CRC, IHDR first, one IDAT, IEND last and empty, nothing behind it."""
    assert data[:8] == SIGNATURE
    at, chunks = 8, []
    while at < len(data):
        (size,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        payload = data[at + 8:at + 8 + size]
        assert len(payload) == size and at + 12 + size <= len(data), kind
        assert struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0] == zlib.crc32(kind + payload), f"the CRC of {kind}"
        chunks.append((kind, payload))
        at += 12 + size
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and chunks[-1][1] == b"" and kinds.count(b"IDAT") == 1 and kinds[-2] == b"IDAT", kinds
    assert all(k == b"tEXt" for k in kinds[1:-2]), kinds
    return chunks


def wrap(chunks):
    """walk's inverse"""
    return SIGNATURE + b"".join(struct.pack(">I", len(p)) + k + p + struct.pack(">I", zlib.crc32(k + p)) for k, p in chunks)


def ihdr(w, h):
    return struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)


def decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


# ---- the restatement of the filters ----------------------------------------------------------------------------------------------------------
def filtered_rows(img):
    """(the five filterings of the uint8 image [H, W, 3] as uint8 [5, H, 3 W], their sums of min(v, 256 - v) as int64 [5, H]): PNG's None, Sub, Up, Average and Paeth
    with bpp = 3; bytes left of a row and above the first row count as 0; mod 256."""
    h, w, _ = img.shape
    x = img.reshape(h, 3 * w).astype(np.int64)
    a = np.zeros_like(x); a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    out = (np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255)
    return out.astype(np.uint8), np.minimum(out, 256 - out).sum(axis=2)


def filtered_data(img, name, rows=None):
    """(F, the rows' types): per row the type byte and the 3 W filtered bytes. "adaptive": the least sum wins, ties to the lowest type (argmin takes the first)."""
    out, score = rows if rows is not None else filtered_rows(img)
    h = img.shape[0]
    types = np.argmin(score, axis=0) if name == "adaptive" else np.full(h, FILTERS.index(name) - 1)
    body = out[types, np.arange(h)]
    return np.concatenate([types.astype(np.uint8)[:, None], body], axis=1).tobytes(), types


def test_the_restatement_is_anchored_to_pil():
    """The yardstick before it judges anything: F built here (each fixed type, and adaptive), deflated by zlib and wrapped by walk's inverse, is a file PIL decodes
    to the pixels it started from; walk accepts it and refuses a damaged one."""
    rng = np.random.default_rng(11)
    for w, h in SMALL + [(7, 5), (33, 12)]:
        img = (rng.integers(0, 256, (h, w, 3)) if w < 33 else (np.add.outer(np.arange(h) * 5, np.arange(w) * 3)[..., None] + rng.integers(0, 4, (h, w, 3))) % 256).astype(np.uint8)
        chosen = set()
        for name in FILTERS:
            f, types = filtered_data(img, name)
            assert len(f) == (3 * w + 1) * h
            data = wrap([(b"IHDR", ihdr(w, h)), (b"tEXt", b"k\0v"), (b"IDAT", zlib.compress(f, 6)), (b"IEND", b"")])
            assert [k for k, _ in walk(data)] == [b"IHDR", b"tEXt", b"IDAT", b"IEND"]
            assert np.array_equal(decode(data), img), (w, h, name)
            chosen |= set(types.tolist()) if name == "adaptive" else set()
        if (w, h) == (33, 12):
            assert len(chosen) >= 2, "the adaptive choice never varied"
    bad = bytearray(data); bad[40] ^= 1
    with pytest.raises(AssertionError):
        walk(bytes(bad))


# ---- the GPU tier ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zctx(pkg, ctx):
    import cray_amd.exrzip as exrzip
    z = exrzip.ZipContext(0)
    assert exrzip.segment_bytes() == SEG
    yield z
    z.close()


def linear_of(bytes8):
    """floats whose 8-bit value is `bytes8`: the middle of each byte's interval, through the inverse of the sRGB curve (checked against to_srgb8 where used)"""
    s = (np.asarray(bytes8, np.float64) + 0.5) / 255.0
    return np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4).astype(np.float32)


def smooth_frame(w, h, seed):
    """a frame with gradients, a little noise, a flat part, a black part and values above 1: rows for which different filters win"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    fb = np.stack([xx / max(w, 2) * 1.2, (xx + yy) / max(w + h, 2), 0.3 + 0.2 * np.sin(yy / 3)], axis=2).astype(np.float32)
    fb += (rng.random((h, w, 3), dtype=np.float32) * 0.02) * (yy[..., None] % 7 < 4)
    fb[(yy % 11 == 5)] = 0.0
    fb[(yy % 13 == 7)] = 0.25
    return np.ascontiguousarray(fb, np.float32)


def check_png(data, w, h, want8, name, rows=None, texts=()):
    """Everything that holds for every file: walk accepts it; IHDR says w x h, 8-bit, colour type 2; PIL's decode equals want8; the inflated IDAT equals the
    restatement's F, type bytes included. Returns the IDAT's payload."""
    chunks = walk(data)
    assert chunks[0][1] == ihdr(w, h)
    assert [p for k, p in chunks if k == b"tEXt"] == [k + b"\0" + v for k, v in texts]
    idat = chunks[-2][1]
    assert idat[:2] == b"\x78\x01"
    got = zlib.decompress(idat)          # (verifies the Adler-32)
    want, types = filtered_data(want8, name, rows)
    assert len(got) == (3 * w + 1) * h
    if got != want:
        first = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"{w} x {h} {name}: F differs first at byte {first} (row {first // (3 * w + 1)}, byte {first % (3 * w + 1)} of it)")
    assert np.array_equal(decode(data), want8), (w, h, name)
    return idat


def pack_all(pkg, ctx, zctx, fb, names=FILTERS, codes=("fixed", "dynamic")):
    """{(filter, codes): the file} for a host frame, each checked by check_png against Context.to_srgb8 of the same device buffer"""
    h, w, _ = fb.shape
    dev = DeviceArray(pkg, fb, np.float32)
    ctx.synchronize()
    want8 = ctx.to_srgb8(dev.ptr, w, h)
    rows = filtered_rows(want8)
    out = {}
    for code in codes:
        zctx.set_codes(code)
        for name in names:
            out[name, code] = zctx.png(dev.ptr, w, h, name)
            check_png(out[name, code], w, h, want8, name, rows)
    zctx.set_codes("fixed")
    assert np.array_equal(dev.read(ctx), fb), "the frame was written"
    return out, want8


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(shape, pkg, ctx, zctx):
    """n = (3 W + 1) H word-unaligned, segments that end mid-row, one segment exactly, one byte more, more segments than the scan's workgroup has lanes: under
    "adaptive" and each fixed type, with both code settings."""
    w, h = shape
    n = (3 * w + 1) * h
    assert {(1, 1): 0, (2, 1): 3, (3, 1): 2, (2, 3): 1}.get(shape, n % 4) == n % 4
    assert {(341, 4): SEG, (80, 17): SEG + 1, (341, 8): 2 * SEG}.get(shape, n) == n and (shape != (400, 880) or -(-n // SEG) > 256)
    files, _ = pack_all(pkg, ctx, zctx, smooth_frame(w, h, 3 * w + h))
    for name in FILTERS:
        assert len(files[name, "dynamic"]) <= len(files[name, "fixed"]), name


def crafted_bytes():
    """uint8 [7, 16, 3]: rows for which, under the rule, each of the five types wins"""
    rng = np.random.default_rng(4)
    w = 16
    img = np.zeros((7, 3 * w), np.int64)
    img[0] = 100                                                   # a constant first row: Sub and Paeth tie at a non-zero sum -> Sub
    img[1] = img[0]                                                # equal to the row above: Up and Paeth tie at zero -> Up
    img[2] = np.repeat(10 + 3 * np.arange(w), 3)                   # a horizontal ramp -> Sub
    for i in range(3 * w):                                         # the average of its neighbours -> Average
        img[3, i] = ((img[3, i - 3] if i >= 3 else 0) + img[2, i]) // 2
    img[4, :24] = rng.integers(0, 256, 24); img[4, 24:] = 200      # noise, then a constant
    img[5, :24] = img[4, :24]; img[5, 24:] = 90                    # the noise again (Up's ground), then another constant (Sub's ground) -> Paeth
    img[6] = np.arange(3 * w) % 2                                  # small values under a large row -> None
    return img.astype(np.uint8).reshape(7, w, 3)


@pytest.mark.gpu
def test_crafted_rows_make_every_type_win(pkg, ctx, zctx):
    """Rows built so that each of the five types wins under the rule — the restatement's choices must cover all five, so the inputs cannot quietly degenerate —, a
    row where two types tie at a non-zero sum, and an all-zero image: a five-way tie that must choose type 0."""
    img = crafted_bytes()
    _, score = filtered_rows(img)
    _, types = filtered_data(img, "adaptive")
    assert types.tolist() == [1, 2, 1, 3, types[4], 4, 0] and set(types.tolist()) == {0, 1, 2, 3, 4}, types
    assert score[1, 0] == score[4, 0] == score[:, 0].min() > 0, "Sub and Paeth tie at a non-zero sum on the first row"
    assert score[2, 1] == score[4, 1] == 0 and score[1, 1] > 0
    files, want8 = pack_all(pkg, ctx, zctx, linear_of(img))
    assert np.array_equal(want8, img), "the floats do not land on the crafted bytes"
    got_types = zlib.decompress(walk(files["adaptive", "fixed"])[-2][1])[::3 * 16 + 1]
    assert list(got_types) == types.tolist()
    black, want8 = pack_all(pkg, ctx, zctx, np.zeros((5, 9, 3), np.float32), names=("adaptive",))
    assert not want8.any() and zlib.decompress(walk(black["adaptive", "dynamic"])[-2][1]) == bytes((3 * 9 + 1) * 5)


@pytest.mark.gpu
def test_values_at_the_conversions_edges(pkg, ctx, zctx):
    """Pixels that land on bytes 0, 1, 254 and 255, the 0.0031308 knee on both sides, values above 1: the file's pixels are to_srgb8's."""
    knee = np.float32(0.0031308)
    values = np.array([0.0, 1e-6, 0.0003, 0.000304, np.nextafter(knee, np.float32(0)), knee, np.nextafter(knee, np.float32(1)), 0.0032, 0.5, 0.99, 0.9911, 0.9913, 0.995, 0.9999,
                       np.nextafter(np.float32(1), np.float32(0)), 1.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, 100.0, 1e30], np.float32)
    values = np.concatenate([values, linear_of([0, 1, 254, 255])])
    fb = np.resize(values, (5, 13, 3)).astype(np.float32)
    _, want8 = pack_all(pkg, ctx, zctx, fb, names=("adaptive", "paeth"))
    assert {0, 1, 254, 255} <= set(want8.reshape(-1).tolist())


@pytest.mark.gpu
def test_rendered_frame_through_write_png(pkg, ctx, zctx, golden_blob, manifest, tmp_path):
    """cfg1_scene at the manifest's size through Context.write_png: the pixels are to_srgb8's, F is the restatement's, the tEXt chunks come back from PIL's info as
    given — an empty value and a 79-byte key among them —, the byte count is the file's, unknown names raise ValueError."""
    m = manifest["cfg1_scene"]
    w, h = m["width"], m["height"]
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    fb = ctx.framebuffer(w, h)
    ctx.render_region(fb, w, h, 4, 4)
    want8 = ctx.to_srgb8(fb, w, h)
    assert len(np.unique(want8)) > 50
    text = {"C-ray Samples": "4", "empty": "", "k" * 79: "a 79-byte key", "Latin": "caf\xe9"}
    sizes = {}
    for name, codes in (("adaptive", "dynamic"), ("adaptive", "fixed"), ("up", "dynamic")):
        path = str(tmp_path / f"{name}_{codes}.png")
        sizes[name, codes] = ctx.write_png(path, w, h, fb, filter=name, codes=codes, text=text)
        data = open(path, "rb").read()
        assert len(data) == sizes[name, codes]
        check_png(data, w, h, want8, name, texts=[(k.encode("latin-1"), v.encode("latin-1")) for k, v in text.items()])
        info = Image.open(io.BytesIO(data)).info
        assert {k: info[k] for k in text} == text
    assert sizes["adaptive", "dynamic"] <= sizes["adaptive", "fixed"] < 3 * w * h
    default = str(tmp_path / "default.png")
    assert ctx.write_png(default, w, h, fb) == sizes["adaptive", "dynamic"] - sum(12 + len(k) + 1 + len(v) for k, v in text.items())
    assert ctx._zip_context().codes == "fixed", "the codes setting is put back"
    for kw in (dict(filter="best"), dict(codes="huffman"), dict(filter=2)):
        with pytest.raises(ValueError):
            ctx.write_png(str(tmp_path / "x.png"), w, h, fb, **kw)
    assert not os.path.exists(str(tmp_path / "x.png"))


@pytest.mark.gpu
def test_crc_alone(zctx):
    """ZipContext.crc32 — the piece CRC and the combination of crx_png_pack on bytes of the caller's — equals zlib.crc32: lengths around the word and the segment,
    pieces of 1, 7 and 4096 bytes, and more pieces than the combining workgroup has lanes."""
    rng = np.random.default_rng(8)
    blob = rng.integers(0, 256, 4097, dtype=np.uint8).tobytes()
    for n in (0, 1, 3, 4, 5, 4095, 4096, 4097):
        for piece in (1, 7, 4096):
            assert zctx.crc32(blob[:n], piece) == zlib.crc32(blob[:n]), (n, piece)
    assert -(-4097 // 7) > 256 and zctx.crc32(bytes(4097), 7) == zlib.crc32(bytes(4097))
    assert zctx.crc32(b"\xff" * 1000, 3) == zlib.crc32(b"\xff" * 1000)
    assert zctx.crc32(b"IEND", 4) == 0xAE426082


def bound_of(zctx, w, h, texts=()):
    import cray_amd.exrzip as exrzip
    arr, count = exrzip.png_texts(texts)
    bound = C.c_uint64(0)
    assert zctx.L.crx_png_bound(w, h, arr, count, C.byref(bound)) == 0
    return bound.value


@pytest.mark.gpu
def test_determinism_and_sizes(pkg, ctx, zctx):
    """Two calls give equal bytes, a call of another shape in between changes nothing; the file is never longer than crx_png_bound, noise under the fixed codes
    included; dynamic codes never give the longer file; an all-black 341 x 8 image's IDAT is under 64 bytes a segment (sixteen maximal matches a segment come to
    about 33 bytes under the fixed codes: a parse that misses the runs fails here)."""
    w, h = 200, 45
    fb = smooth_frame(w, h, 1)
    first, _ = pack_all(pkg, ctx, zctx, fb, names=("adaptive", "sub"))
    pack_all(pkg, ctx, zctx, smooth_frame(3, 1, 2), names=("adaptive",))
    again, _ = pack_all(pkg, ctx, zctx, fb, names=("adaptive", "sub"))
    assert first == again
    segs = -(-(3 * w + 1) * h // SEG)
    assert bound_of(zctx, w, h) == 8 + 25 + 12 + 2 + segs * 4640 + 4 + 12
    assert bound_of(zctx, w, h, [("ab", "cde")]) == bound_of(zctx, w, h) + 12 + 2 + 1 + 3
    for key, data in first.items():
        assert len(data) <= bound_of(zctx, w, h), key
    for name in ("adaptive", "sub"):
        assert len(first[name, "dynamic"]) <= len(first[name, "fixed"])
    noise = np.random.default_rng(6).random((40, 64, 3), dtype=np.float32)
    files, _ = pack_all(pkg, ctx, zctx, noise, names=("none", "adaptive"))
    assert all(len(d) <= bound_of(zctx, 64, 40) for d in files.values())
    black, _ = pack_all(pkg, ctx, zctx, np.zeros((8, 341, 3), np.float32), names=("adaptive", "none", "paeth"))
    for key, data in black.items():
        assert len(walk(data)[-2][1]) < 64 * 2, (key, len(walk(data)[-2][1]))


@pytest.mark.gpu
def test_refused_arguments_leave_everything_untouched(pkg, ctx, zctx):
    """CRH_ERR_INVALID for every refusal of the header; the poisoned output and total_bytes stay as they were; the context works afterwards."""
    import cray_amd.exrzip as exrzip
    abi, L = pkg.abi, zctx.L
    w, h = 20, 6
    fb = smooth_frame(w, h, 9)
    dev = DeviceArray(pkg, fb, np.float32)
    ctx.synchronize()
    bound = bound_of(zctx, w, h, [("key", "value")])
    out = np.full(bound, 0xA5, np.uint8)
    total = C.c_uint64(0x5A5A5A5A5A5A5A5A)
    good = [(b"key", b"value")]

    def call(handle=zctx.h, src=dev.ptr, width=w, height=h, filt=-1, texts=good, count=None, null_list=False, dst=out.ctypes.data, capacity=bound, tot=C.byref(total)):
        arr = (exrzip.PngText * max(len(texts), 1))(*[exrzip.PngText(k, v) for k, v in texts])
        return L.crx_png_pack(handle, src, width, height, filt, None if null_list else arr, len(texts) if count is None else count, dst, capacity, tot)
    refused = {
        "NULL context": dict(handle=None), "NULL frame": dict(src=None), "NULL output": dict(dst=None), "NULL total": dict(tot=None),
        "width 0": dict(width=0), "height 0": dict(height=0), "width < 0": dict(width=-w), "height < 0": dict(height=-h),
        "n = 2^31": dict(width=(2 ** 31 // 64 - 1) // 3 + 1, height=64, capacity=2 ** 62), "n far above 2^31": dict(width=2 ** 30, height=2 ** 30, capacity=2 ** 62),
        "filter -2": dict(filt=-2), "filter 5": dict(filt=5),
        "a NULL list with a count": dict(null_list=True, count=1), "an empty key": dict(texts=[(b"", b"v")]), "a key of 80 bytes": dict(texts=[(b"k" * 80, b"v")]),
        "a NULL key": dict(texts=[(None, b"v")]), "a NULL value": dict(texts=good + [(b"k", None)]),
        "capacity below the bound": dict(capacity=bound - 1), "capacity 0": dict(capacity=0),
    }
    for what, kw in refused.items():
        assert call(**kw) == abi.ERR_INVALID, what
        assert b"crx_png_pack" in L.crx_last_error(), what
        assert (out == 0xA5).all() and total.value == 0x5A5A5A5A5A5A5A5A, what
    value = C.c_uint64(7)
    for kw in (dict(width=0), dict(height=-1), dict(width=2 ** 30, height=2 ** 30)):
        assert L.crx_png_bound(kw.get("width", w), kw.get("height", h), None, 0, C.byref(value)) == abi.ERR_INVALID and value.value == 7
    assert L.crx_png_bound(w, h, None, 1, C.byref(value)) == abi.ERR_INVALID and L.crx_png_bound(w, h, None, 0, None) == abi.ERR_INVALID
    crc = C.c_uint32(7)
    assert L.crx_debug_crc32(zctx.h, b"abc", 3, 0, C.byref(crc)) == abi.ERR_INVALID and L.crx_debug_crc32(zctx.h, None, 3, 1, C.byref(crc)) == abi.ERR_INVALID and crc.value == 7
    # the context works afterwards; nothing behind the file is written
    assert call() == abi.OK
    data = out[:total.value].tobytes()
    check_png(data, w, h, ctx.to_srgb8(dev.ptr, w, h), "adaptive", texts=good)
    assert total.value <= bound and (out[total.value:] == 0xA5).all()
    assert call(texts=[], count=0, null_list=True) == abi.OK, "a NULL list with a count of zero is no text"
    assert len(zctx.png_phases_ms()) == 5 and sum(zctx.png_phases_ms()) >= 0.0


def run_dropin_png(manifest, out_dir, env):
    """support.run_dropin with the frame's own file a PNG: c-ray-hip on cfg1_scene, {file name: bytes} of out_dir and the program's output"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import refrun
    exe, overlay, _ = dropin_paths()
    m = manifest["cfg1_scene"]
    os.makedirs(out_dir, exist_ok=True)
    scene = refrun.rewrite_scene("scene.json", m["width"], m["height"], m["samples"], m["bounces"], out_dir=str(out_dir), file_type="png")
    child = {k: v for k, v in os.environ.items() if not k.startswith("CRAY_HIP_") and k not in ("CRH_DENOISE_FORM", "CRH_DROPIN_PASSES")}
    child["CRAY_HIP_DEVICES"] = "1"
    child.update(env)
    proc = subprocess.run([exe], input=json.dumps(scene).encode(), cwd=overlay, env=child, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = proc.stdout.decode(errors="replace")
    assert proc.returncode == 0, text[-2000:]
    return {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}, text


@pytest.mark.gpu
def test_dropin_program_writes_the_gpu_png(manifest, tmp_path):
    """c-ray-hip with CRAY_HIP_PNG=1: <name>_gpu_0000.png stands next to the frame's own PNG, PIL decodes both to the same pixels, the tEXt chunks name the samples
    and the bounces, one log line gives the size; without the variable no such file appears and the frame's own file is the same."""
    if not dropin_paths()[2]:
        pytest.skip("c-ray-hip or the asset overlay is not built (needs the reference's sources at build time)")
    m = manifest["cfg1_scene"]
    plain, _ = run_dropin_png(manifest, str(tmp_path / "plain"), dropin_env())
    files, text = run_dropin_png(manifest, str(tmp_path / "png"), dict(dropin_env(), CRAY_HIP_PNG="1"))
    assert "refrun_0000.png" in plain and not [f for f in plain if "_gpu_" in f]
    assert sorted(files) == sorted(list(plain) + ["refrun_gpu_0000.png"])
    assert np.array_equal(decode(files["refrun_0000.png"]), decode(plain["refrun_0000.png"]))          # (the reference's own file carries the run's render time)
    data = files["refrun_gpu_0000.png"]
    chunks = walk(data)
    assert chunks[0][1] == ihdr(m["width"], m["height"])
    assert [p for k, p in chunks if k == b"tEXt"] == [b"C-ray Samples\0" + str(m["samples"]).encode(), b"C-ray Bounces\0" + str(m["bounces"]).encode()]
    assert np.array_equal(decode(data), decode(files["refrun_0000.png"]))
    assert f"refrun_gpu_0000.png: {len(data)} bytes" in text, text[-1500:]
    fixed, _ = run_dropin_png(manifest, str(tmp_path / "fixed"), dict(dropin_env(), CRAY_HIP_PNG="1", CRAY_HIP_EXR_CODES="fixed"))
    assert len(fixed["refrun_gpu_0000.png"]) >= len(data) and np.array_equal(decode(fixed["refrun_gpu_0000.png"]), decode(data))


# ---- the CPU tier's run of the above ------------------------------------------------------------------------------------------------------
def test_png_kernels_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the emulation builds — tests/emu/libcray_hip_exr_emu.so (Makefile.exr: exr_zip.hip with
    png_pack.h, unmodified, on the HIP-on-CPU shim) beside tests/emu/libcray_hip_emu.so —: every one of them runs and passes there, none skipped (the drop-in test
    where the drop-in program is built)."""
    run_gpu_tests_on_emulation(__file__, 16, passed_without_dropin=15, extra_env={"CRX_LIB": os.path.join(EMU_DIR, "libcray_hip_exr_emu.so")},
                               make_targets=("libcray_hip_emu.so", "-f Makefile.exr"), dropin_libs=("libcray_hip_exr.so",))
