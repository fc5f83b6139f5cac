"""The layers file, ZIP / ZIPS compressed on the device: crx_pack_zip of the companion library libcray_hip_exr.so (include/cray_hip_exr.h, c-ray_amd/csrc/exr_zip.h)
gathers the channels crh_pack_scanlines gathers, applies OpenEXR's byte split and predictor and deflates every chunk with fixed Huffman codes;
exr.file_bytes and exr_write_file (c-ray_amd/host/exr_write.c) write the file around the chunks.

The reader (tests/exr_reader.py: it inflates with Python's zlib, undoes the predictor and the split and checks the offset table against the chunk positions) is
anchored here by a 2 x 1 ZIPS file spelled out field by field. CPU tier: the format, the Python writer, the C writer against it, and this file's
GPU tests run by a child pytest on the emulation (tests/emu/Makefile.exr). GPU tier: the inflated chunks bit for bit against Context.pack_scanlines, crafted
planes, chunked calls, refused arguments, size conditions against host zlib with fixed codes, a rendered file, the drop-in program."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from exr_reader import (ALL_38, LINES, check_crypto_layer, flat_source, hand_built_2x1, host_chunks, inflate_chunk, raw_of, read_exr, run_dropin, split_chunks, strip_headers,
                        zip_case, zip_forward, zip_inverse)
from firsthit_spec import resolve_expected
from support import EMU_DIR, REPO, DeviceArray, ctx, dropin_env, dropin_paths, run_gpu_tests_on_emulation  # noqa: F401 (ctx: the fixture)


def yardstick(raw, n_per_chunk):
    """host zlib with fixed codes (level 1, Z_FIXED) per chunk on the same T', raw where that is not shorter: (bytes with the 8-byte headers, raw bytes with them)"""
    got = want = 0
    for at in range(0, len(raw), n_per_chunk):
        r = raw[at:at + n_per_chunk]
        c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        z = c.compress(zip_forward(r)) + c.flush()
        got += 8 + min(len(z), len(r))
        want += 8 + len(r)
    return got, want


# ---- CPU tier: the format ---------------------------------------------------------------------------------------------------------------
def hand_built_2x1_zips():
    """The 2 x 1 image of exr_reader.hand_built_2x1— B = (0.25, -0.0), R = (1.5, NaN 0x7fc00123) — as a ZIPS file: one chunk, raw (16 bytes do not deflate)."""
    def attr(name, kind, value):
        return name + b"\0" + kind + b"\0" + struct.pack("<i", len(value)) + value

    def channel(name):
        return name + b"\0" + struct.pack("<i", 2) + struct.pack("<B", 0) + b"\0\0\0" + struct.pack("<i", 1) + struct.pack("<i", 1)
    head = bytes([0x76, 0x2F, 0x31, 0x01]) + bytes([0x02, 0x00, 0x00, 0x00])
    head += attr(b"channels", b"chlist", channel(b"B") + channel(b"R") + b"\0")
    head += attr(b"compression", b"compression", struct.pack("<B", 2))
    head += attr(b"dataWindow", b"box2i", struct.pack("<4i", 0, 0, 1, 0))
    head += attr(b"displayWindow", b"box2i", struct.pack("<4i", 0, 0, 1, 0))
    head += attr(b"lineOrder", b"lineOrder", struct.pack("<B", 0))
    head += attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
    head += attr(b"screenWindowCenter", b"v2f", struct.pack("<2f", 0.0, 0.0))
    head += attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0))
    head += b"\0"
    raw = struct.pack("<4I", 0x3E800000, 0x80000000, 0x3FC00000, 0x7FC00123)
    # the transform by hand: R = 00 00 80 3e | 00 00 00 80 | 00 00 c0 3f | 23 01 c0 7f; even bytes 00 80 00 00 00 c0 23 c0, odd bytes 00 3e 00 80 00 3f 01 7f
    t = bytes([0x00, 0x80, 0x00, 0x00, 0x00, 0xC0, 0x23, 0xC0, 0x00, 0x3E, 0x00, 0x80, 0x00, 0x3F, 0x01, 0x7F])
    tp = bytes([t[0]] + [(t[j] - t[j - 1] + 128) & 255 for j in range(1, 16)])
    assert tp == bytes([0x00, 0x00, 0x00, 0x80, 0x80, 0x40, 0xE3, 0x1D, 0xC0, 0xBE, 0x42, 0x00, 0x00, 0xBF, 0x42, 0xFE])
    z = zlib.compress(tp, 9)
    assert len(z) >= 16, "16 bytes with no repeats do not deflate: the chunk is raw"
    chunk = struct.pack("<i", 0) + struct.pack("<i", 16) + raw
    return head + struct.pack("<Q", len(head) + 8) + chunk, tp


def test_reader_is_anchored_and_exr_py_writes_the_chunked_file(pkg):
    exr = pkg.exr
    data, tp = hand_built_2x1_zips()
    assert zip_forward(struct.pack("<4I", 0x3E800000, 0x80000000, 0x3FC00000, 0x7FC00123)) == tp and zip_inverse(tp) == data[-16:]
    f = read_exr(data)
    assert (f["width"], f["height"], f["names"], f["compression"]) == (2, 1, ["B", "R"], 2)
    assert f["planes"]["B"].tolist() == [[0x3E800000, 0x80000000]] and f["planes"]["R"].tolist() == [[0x3FC00000, 0x7FC00123]]
    b, r = np.array([[0x3E800000, 0x80000000]], np.uint32), np.array([[0x3FC00000, 0x7FC00123]], np.uint32)
    chunks, sizes = host_chunks([b, r], 2, 1, 2)
    assert sizes == [24]
    assert exr.file_bytes(2, 1, ["B", "R"], chunks, sizes, compression=2) == data
    # compression 0 keeps its bytes
    assert exr.file_bytes(2, 1, ["B", "R"], exr.pack_host([b, r], 2, 1)) == hand_built_2x1()
    assert exr.header(2, 1, ["B", "R"]) == exr.header(2, 1, ["B", "R"], compression=0) == hand_built_2x1()[:-8 - 24]
    # a compressible image of two ZIP chunks (17 rows) and of 17 ZIPS chunks: deflated chunks, a short last chunk, strings
    rng = np.random.default_rng(5)
    planes = [np.repeat(rng.integers(0, 2 ** 32, (17, 5), dtype=np.uint32), 8, axis=1) for _ in range(3)]
    for kind in (2, 3):
        chunks, sizes = host_chunks(planes, 40, 17, kind)
        whole = exr.file_bytes(40, 17, ["A", "B", "C"], chunks, sizes, {"zzz": "ä"}, kind)
        g = read_exr(whole)
        assert g["compression"] == kind and len(g["chunks"]) == (17 if kind == 2 else 2) and any(size < n for _, size, n in g["chunks"])
        for name, p in zip("ABC", planes):
            assert np.array_equal(g["planes"][name], p)
        assert g["attrs"]["zzz"] == ("string", "ä".encode())
    with pytest.raises(AssertionError):
        exr.file_bytes(40, 17, ["A", "B", "C"], chunks, sizes[:-1], None, 3)          # a chunk short
    # compression 0 without types is the flat file: its chunks are the packer's blocks, with their sizes stated or left out
    assert exr.file_bytes(2, 1, ["B", "R"], exr.pack_host([b, r], 2, 1), [24], compression=0) == hand_built_2x1()
    with pytest.raises(AssertionError):
        exr.file_bytes(40, 17, ["A", "B", "C"], chunks, None, None, 3)          # only compression 0 says what its chunks' sizes are


C_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "exr_write.h"
/* argv: out width height compression chunk-file size... — the chunks come from the file, their sizes from the command line */
int main(int argc, char **argv) {
	static const char *names[3] = {"A", "B", "C"};
	struct exr_attr strings[2] = {{"aaa", ""}, {"zzz", "\303\244 \"q\""}};
	if (argc < 7) return 1;
	const int w = atoi(argv[2]), h = atoi(argv[3]), kind = atoi(argv[4]), count = argc - 6;
	uint64_t *sizes = malloc((size_t)count * sizeof(*sizes));
	uint64_t total = 0;
	for (int k = 0; k < count; ++k) { sizes[k] = strtoull(argv[6 + k], NULL, 10); total += sizes[k]; }
	unsigned char *data = malloc(total ? total : 1);
	FILE *f = fopen(argv[5], "rb");
	if (!f || fread(data, 1, total, f) != total) return 3;
	fclose(f);
	const int rc = exr_write_file(argv[1], w, h, names, NULL, 3, strings, 2, kind, data, sizes, count);
	const int refused = exr_write_file(argv[1], w, h, names, NULL, 3, strings, 2, kind, data, sizes, count - 1) == 0 ||
	                    exr_write_file(argv[1], w, h, names, NULL, 3, strings, 2, 1, data, sizes, count) == 0;
	free(sizes); free(data);
	return rc ? 2 : refused ? 4 : 0;
}
"""


def test_c_chunked_writer_writes_the_bytes_of_exr_py(pkg, tmp_path):
    """exr_write_file in a program of its own (AddressSanitizer and UBSan) against exr.file_bytes, byte for byte: ZIP and ZIPS, host-made chunks
    with a raw-fallback chunk (random rows) among deflated ones and a short last chunk; a wrong chunk count and a wrong compression are refused."""
    exr = pkg.exr
    host = os.path.join(REPO, "c-ray_amd", "host")
    src, exe = tmp_path / "zc.c", tmp_path / "zc"
    src.write_text(C_PROGRAM)
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(REPO, "include"), "-I" + host, str(src), os.path.join(host, "exr_write.c"), "-o", str(exe)])
    rng = np.random.default_rng(9)
    w, h = 24, 35
    planes = [np.repeat(rng.integers(0, 2 ** 32, (h, 3), dtype=np.uint32), 8, axis=1) for _ in range(3)]
    for p in planes:
        p[16:32] = rng.integers(0, 2 ** 32, (16, w), dtype=np.uint32)          # the second ZIP chunk and rows 16 .. 31 do not deflate
    for kind in (2, 3):
        chunks, sizes = host_chunks(planes, w, h, kind)
        n = 4 * 3 * w * LINES[kind]
        assert (8 + n) in sizes and min(sizes) < 8 + n // 2 and (kind == 2 or sizes[-1] < 8 + 4 * 3 * w * 3), "a raw chunk, deflated ones, a short last one"
        blob, out = tmp_path / f"chunks{kind}", tmp_path / f"c{kind}.exr"
        blob.write_bytes(chunks)
        r = subprocess.run([str(exe), str(out), str(w), str(h), str(kind), str(blob)] + [str(s) for s in sizes], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        want = exr.file_bytes(w, h, ["A", "B", "C"], chunks, sizes, {"aaa": "", "zzz": "ä \"q\""}, kind)
        got = out.read_bytes()
        assert got == want
        f = read_exr(got)
        for name, p in zip("ABC", planes):
            assert np.array_equal(f["planes"][name], p)


# ---- the GPU tier -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zctx(pkg, ctx):
    import cray_amd.exrzip as exrzip
    z = exrzip.ZipContext(0)
    yield z
    z.close()


def seg():
    import cray_amd.exrzip as exrzip
    return exrzip.segment_bytes()


def run_zip(pkg, ctx, zctx, case, lines, **rows):
    """(crx_pack_zip's bytes, its sizes, the raw bytes Context.pack_scanlines gives for the same rows with the row headers stripped)"""
    w, h, src, chans, maps = case
    dev = {k: DeviceArray(pkg, v, np.uint32) for k, v in src.items()}
    ch = [(dev[k].ptr, stride, comp, None if m is None else maps[m]) for k, stride, comp, m in chans]
    ctx.synchronize()
    data, sizes = zctx.pack_zip(ch, w, h, lines, **rows)
    want = strip_headers(ctx.pack_scanlines(ch, w, h, **rows), len(chans), w)
    for k, d in dev.items():
        assert np.array_equal(d.read(ctx), src[k]), "a source was written"
    return data, sizes, want


def shapes():
    s = seg() // 4          # words of a segment
    def split(words):          # words -> (w, nch) with nch <= 64
        for nch in range(1, 65):
            if words % nch == 0 and words // nch <= 700:
                return words // nch, nch
        raise AssertionError(words)
    out = ["1x1x1", "3x2x7", "67x5x3", "40x16x5", "40x17x5", "9x75x2", "161x75x38"]
    for words in (s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1):          # a ZIPS chunk of S - 4, S, S + 4, 2 S - 4, 2 S, 2 S + 4 bytes
        w, nch = split(words)
        out.append(f"{w}x3x{nch}")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("lines", [1, 16])
def test_round_trip_against_the_packer(lines, pkg, ctx, zctx):
    """Every chunk inflated and un-transformed is, bit for bit, what Context.pack_scanlines packs for the same channels: NaN payloads, -0.0, subnormals, ids out of
    range; 1 x 1 x 1 comes back raw; heights 16, 17 and 75 end in a ZIP chunk of 16, 1 and 11 lines; chunks of S - 4 .. 2 S + 4 bytes."""
    for name in shapes():
        case = zip_case(name)
        w, h, nch = case[0], case[1], len(case[3])
        data, sizes, want = run_zip(pkg, ctx, zctx, case, lines)
        chunks = split_chunks(data, sizes, 4 * nch * w, 0, h, lines)
        got = raw_of(chunks)
        assert got == want, name
        assert int(sizes.sum()) == len(data) and all(8 + len(d) <= 8 + n for _, d, n in chunks)
        if name == "1x1x1":
            assert len(data) == 12 and chunks[0][1] == want, "4 bytes come back raw"
        elif w * nch >= 60:
            assert any(len(d) < n for _, d, n in chunks), name + ": nothing deflated"
        if name == "40x17x5" and lines == 16:
            assert [n for _, _, n in chunks] == [4 * 5 * 40 * 16, 4 * 5 * 40]
        if name == "161x75x38":
            assert zctx.time_ms() > 0.0 and len(zctx.phases_ms()) == 4


def crafted(tps):
    """transformed chunks of equal size -> the one-channel planes [chunks, n / 4] whose ZIPS chunk k has T' = tps[k]"""
    n = len(tps[0])
    assert n % 4 == 0 and all(len(t) == n for t in tps)
    return np.stack([np.frombuffer(zip_inverse(t), "<u4") for t in tps]).astype(np.uint32)


def backdrop(n):
    """n bytes that deflate but hold no run and no period below 7: what the crafted stretches are set into, so that their chunks take the deflate path"""
    return np.resize(np.array([1, 2, 3, 4, 5, 6, 7], np.uint8), n).copy()


@pytest.mark.gpu
def test_crafted_planes(pkg, ctx, zctx):
    """Planes whose TRANSFORMED bytes have the property (built as T', inverted on the host): runs of exactly 258 .. 261 equal bytes, a period-2 and a period-3
    pattern across a segment boundary, a repeat at the largest distance a segment allows, literals on both sides of 143 / 144, and a chunk of pseudo-random bytes
    between two compressible ones — raw in the middle of a file."""
    S = seg()
    rng = np.random.default_rng(77)
    n = 2 * S + 8
    tps, what = [], []
    for run in (258, 259, 260, 261):          # a run starts behind 100 other bytes; what follows differs
        t = backdrop(n)
        t[100:100 + run] = 0x55
        tps.append(t.tobytes()); what.append(f"run {run}")
    for period in (2, 3):          # S - 150 .. S + 150
        t = backdrop(n)
        t[S - 150:S + 150] = np.resize(np.array([77, 200, 91][:period], np.uint8), 300)
        tps.append(t.tobytes()); what.append(f"period {period}")
    marker = rng.integers(8, 256, 12, dtype=np.uint8)
    for k, name in enumerate(("largest distance", "no repeat")):          # the first 12 bytes of the second segment again at its end: distance S - 12
        t = backdrop(n)
        t[S:S + 12] = marker
        t[2 * S - 12:2 * S] = marker if k == 0 else marker[::-1] ^ 0x80
        tps.append(t.tobytes()); what.append(name)
    t = np.resize(np.array([141, 142, 143, 144, 145, 0, 255, 143, 144, 143, 143, 144, 144], np.uint8), n)
    t[::11] = rng.integers(0, 256, t[::11].size, dtype=np.uint8)          # (so that not everything is one match)
    tps.append(t.tobytes()); what.append("literals around 143 / 144")
    tps.append(bytes(n)); what.append("zeros")
    tps.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes()); what.append("random")
    tps.append(bytes([128]) * n); what.append("constant")
    planes = crafted(tps)
    h, w = planes.shape
    dev = DeviceArray(pkg, planes.reshape(h, w, 1), np.uint32)
    ctx.synchronize()
    data, sizes = zctx.pack_zip([(dev.ptr, 1, 0)], w, h, 1)
    chunks = split_chunks(data, sizes, 4 * w, 0, h, 1)
    for k, (y, d, nn) in enumerate(chunks):
        assert inflate_chunk(d, nn) == planes[k].astype("<u4").tobytes(), what[k]
        if len(d) < nn:
            assert zlib.decompress(d) == tps[k], what[k]
    size = {name: len(d) for name, (_, d, _) in zip(what, chunks)}
    assert size["random"] == n and size["zeros"] < 120 and size["constant"] < 120, size          # raw between two chunks of a few dozen bytes
    assert size["literals around 143 / 144"] < n and all(v < n // 4 for k, v in size.items() if k not in ("random", "literals around 143 / 144")), size          # all deflated
    assert size["largest distance"] <= size["no repeat"] - 6, size                                # twelve literals became one match
    # ZIP: the same planes as chunks of 16 rows (the last of 11 - 16 rows): every byte again
    data16, sizes16 = zctx.pack_zip([(dev.ptr, 1, 0)], w, h, 16)
    assert raw_of(split_chunks(data16, sizes16, 4 * w, 0, h, 16)) == planes.astype("<u4").tobytes()


@pytest.mark.gpu
def test_determinism_and_chunked_calls(pkg, ctx, zctx):
    """The same call twice gives equal bytes; first_row ranges of 16, 32 and the rest concatenate to the single call's bytes and sizes; the sizes add up."""
    case = zip_case("67x75x9")
    w, h, nch = case[0], case[1], len(case[3])
    for lines in (1, 16):
        whole, sizes, want = run_zip(pkg, ctx, zctx, case, lines)
        again, sizes2, _ = run_zip(pkg, ctx, zctx, case, lines)
        assert whole == again and np.array_equal(sizes, sizes2)
        assert int(sizes.sum()) == len(whole)
        parts = [run_zip(pkg, ctx, zctx, case, lines, first_row=f, row_count=r) for f, r in ((0, 16), (16, 32), (48, h - 48))]
        assert b"".join(p[0] for p in parts) == whole
        assert np.array_equal(np.concatenate([p[1] for p in parts]), sizes)
        for (data, sz, raw), (f, r) in zip(parts, ((0, 16), (16, 32), (48, h - 48))):
            assert raw_of(split_chunks(data, sz, 4 * nch * w, f, r, lines)) == raw
        # a call of another shape in between changes nothing
        run_zip(pkg, ctx, zctx, zip_case("3x2x7"), lines)
        assert run_zip(pkg, ctx, zctx, case, lines)[0] == whole


@pytest.mark.gpu
def test_refused_arguments_leave_everything_untouched(pkg, ctx, zctx):
    """CRH_ERR_INVALID for every refusal of the header; the output and both size outputs keep the pattern they were filled with; the next valid call works."""
    abi = pkg.abi
    w, h = 40, 35
    rng = np.random.default_rng(3)
    a, b = DeviceArray(pkg, flat_source(rng, w, h, 3), np.uint32), DeviceArray(pkg, flat_source(rng, w, h, 8), np.uint32)
    m = np.arange(7, dtype=np.uint32)
    good = [(a.ptr, 3, 1, None, 0), (b.ptr, 8, 7, m.ctypes.data, 7)]
    out = np.full(8 * h + 4 * 2 * w * h, 0xA5, np.uint8)
    sizes = np.full(h, 0xA5A5A5A5A5A5A5A5, np.uint64)
    total = C.c_uint64(0x5A5A5A5A5A5A5A5A)
    L = zctx.L

    def call(chans=good, count=None, width=w, height=h, first=0, rows=h, lines=16, handle=zctx.h, dst=out.ctypes.data, null_list=False, sz=sizes.ctypes.data, tot=C.byref(total)):
        arr = (abi.PackChannel * 66)()
        for k, c in zip(arr, chans):
            k.dev_src, k.stride, k.component, k.map_host, k.map_count = c
        return L.crx_pack_zip(handle, None if null_list else arr, len(chans) if count is None else count, width, height, first, rows, lines, dst, sz, tot)
    refused = {
        "NULL context": dict(handle=None), "NULL list": dict(null_list=True), "NULL output": dict(dst=None), "NULL sizes": dict(sz=None), "NULL total": dict(tot=None),
        "NULL source": dict(chans=[good[0], (None, 3, 0, None, 0)]), "no channels": dict(count=0), "65 channels": dict(chans=[good[0]] * 65),
        "width 0": dict(width=0), "height 0": dict(height=0), "width < 0": dict(width=-w), "height < 0": dict(height=-h),
        "first_row < 0": dict(first=-16, rows=16), "row_count < 0": dict(rows=-1), "rows past the image": dict(first=16, rows=h), "first_row == height": dict(first=h, rows=1, lines=1),
        "component == stride": dict(chans=[(a.ptr, 3, 3, None, 0)]), "stride 0": dict(chans=[(a.ptr, 0, 0, None, 0)]), "stride 65": dict(chans=[(a.ptr, 65, 0, None, 0)]),
        "map_count 65537": dict(chans=[good[0], (b.ptr, 8, 7, m.ctypes.data, 65537)]), "a map with count 0": dict(chans=[(b.ptr, 8, 7, m.ctypes.data, 0)]),
        "lines_per_chunk 0": dict(lines=0), "lines_per_chunk 2": dict(lines=2), "lines_per_chunk 32": dict(lines=32), "lines_per_chunk -16": dict(lines=-16),
        "first_row off the chunks": dict(first=8, rows=h - 8), "an end off the chunks": dict(first=0, rows=20), "an end off the chunks, from 16": dict(first=16, rows=3),
        "a chunk of 2^31 bytes": dict(chans=[good[0]] * 64, width=(1 << 31) // (4 * 64 * 16), height=16, rows=16),
    }
    for what, kw in refused.items():
        assert call(**kw) == abi.ERR_INVALID, what
        assert b"crx_pack_zip" in L.crx_last_error(), what
        assert (out == 0xA5).all() and (sizes == 0xA5A5A5A5A5A5A5A5).all() and total.value == 0x5A5A5A5A5A5A5A5A, what
    # row_count == 0: CRH_OK, nothing written but the total
    for first in (0, 16, 32):
        assert call(first=first, rows=0) == abi.OK and total.value == 0
        assert (out == 0xA5).all() and (sizes == 0xA5A5A5A5A5A5A5A5).all()
        total.value = 0x5A5A5A5A5A5A5A5A
    assert call() == abi.OK
    chunks = split_chunks(out[:total.value].tobytes(), sizes[:3], 4 * 2 * w, 0, h, 16)
    want = strip_headers(ctx.pack_scanlines([(a.ptr, 3, 1), (b.ptr, 8, 7, m)], w, h), 2, w)
    assert raw_of(chunks) == want
    assert (out[total.value:] == 0xA5).all() and (sizes[3:] == 0xA5A5A5A5A5A5A5A5).all(), "nothing behind the chunks is written"


def size_sets():
    """the planes of the size conditions, all 160 x 96"""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:96, 0:160]
    blob = xx // 23 + (yy // 17) * 7
    edge = (xx % 23 == 0) | (yy % 17 == 0)
    ids = ((blob.astype(np.uint64) * 2654435761) % 2 ** 32).astype(np.uint32) | 0x3F000000
    cov = np.ones((96, 160), np.float32)
    cov[edge] = (rng.integers(1, 16, int(edge.sum())) / 16).astype(np.float32)
    const = [np.full((96, 160), v, np.float32) for v in (0.0, 1.0, 0.25, -3.5)]
    noise = [rng.random((96, 160), dtype=np.float32) for _ in range(3)]
    guides = [(np.sin(xx / 30 + k) + yy / 50).astype(np.float32) for k in range(6)] + [cov, ((blob % 5) / 4).astype(np.float32)]
    matte = [ids, cov, np.where(edge, ids, np.uint32(0)).astype(np.uint32), (1 - cov).astype(np.float32), np.zeros((96, 160), np.float32), np.zeros((96, 160), np.float32)]
    mixed = noise + guides + matte + matte
    assert len(mixed) == 23
    return {"const": const, "noise": noise, "mixed": mixed}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["const", "mixed", "noise"])
def test_size_conditions(name, pkg, ctx, zctx):
    """Shares of the raw size (chunk headers on both sides). The yardstick — host zlib, level 1, fixed codes, per chunk on the same T', raw where not shorter — is
    asserted first, so the input is known to be adequate; then the device: const <= 0.05 (yardstick within 0.03), mixed <= 0.40 (within 0.30), noise all raw."""
    planes = [np.ascontiguousarray(p).view(np.uint32) for p in size_sets()[name]]
    w, h, nch = 160, 96, len(planes)
    words = np.ascontiguousarray(np.stack(planes, axis=2))          # [h, w, nch]
    dev = DeviceArray(pkg, words, np.uint32)
    ch = [(dev.ptr, nch, c) for c in range(nch)]
    ctx.synchronize()
    raw = strip_headers(ctx.pack_scanlines(ch, w, h), nch, w)
    assert raw == np.stack(planes, axis=1).astype("<u4").tobytes()
    for lines in (1, 16):
        n = 4 * nch * w * lines
        ygot, ywant = yardstick(raw, n)
        data, sizes = zctx.pack_zip(ch, w, h, lines)
        chunks = split_chunks(data, sizes, 4 * nch * w, 0, h, lines)
        assert raw_of(chunks) == raw
        share, yshare = len(data) / ywant, ygot / ywant
        print(f"{name} lines {lines}: yardstick {yshare:.4f}, device {share:.4f} of {ywant} bytes, segment {seg()}")
        assert all(len(d) <= nn for _, d, nn in chunks)
        if name == "const":
            assert yshare <= 0.03 and share <= 0.05, (yshare, share)
        elif name == "mixed":
            assert yshare <= 0.30 and share <= 0.40, (yshare, share)
        else:
            assert ygot == ywant, "the yardstick leaves noise raw"
            assert len(data) == ywant and all(len(d) == nn for _, d, nn in chunks), "every chunk raw"


@pytest.mark.gpu
def test_rendered_layers_file_compressed(pkg, ctx, golden_blob, manifest, tmp_path):
    """cfg1_scene at the manifest's size with the frame, the guides, a denoised frame and both ID buffers, written with compression "none", "zip" and "zips": the
    compressed files parse, every plane equals the uncompressed file's bit for bit, the Cryptomatte attributes are identical, and the files are smaller — after
    the zlib yardstick over the same chunks has been seen to be smaller."""
    m = manifest["cfg1_scene"]
    w, h, n = m["width"], m["height"], 4
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    fb, dn, aov = ctx.framebuffer(w, h), ctx.framebuffer(w, h), ctx.aov_buffer(w, h)
    bi, bm = ctx.ids_buffer(w, h), ctx.ids_buffer(w, h)
    ctx.render_region(fb, w, h, n, 4)
    ctx.render_aov(aov, w, h, n)
    ctx.render_ids(bi, bm, w, h, n)
    ctx.denoise(fb, aov, w, h, out=dn, iterations=2)
    kw = dict(aov=aov, denoised=dn, instance_ids=bi, material_ids=bm)
    plain_path = str(tmp_path / "none.exr")
    names = ctx.write_layers_exr(plain_path, w, h, fb, compression="none", **kw)
    plain = open(plain_path, "rb").read()
    ctx.write_layers_exr(str(tmp_path / "default.exr"), w, h, fb, **kw)
    assert open(str(tmp_path / "default.exr"), "rb").read() == plain, '"none" is the default and today\'s bytes'
    f0 = read_exr(plain)
    assert f0["compression"] == 0 and f0["names"] == names == sorted(ALL_38, key=lambda s: s.encode())
    raw = np.stack([f0["planes"][c] for c in names], axis=1).astype("<u4").tobytes()          # [H, C, W]
    for compression, kind, chunk_rows in (("zip", 3, 40), ("zips", 2, 37), ("zip", 3, None)):
        path = str(tmp_path / (compression + ".exr"))
        assert ctx.write_layers_exr(path, w, h, fb, compression=compression, chunk_rows=chunk_rows, **kw) == names
        data = open(path, "rb").read()
        f = read_exr(data)
        assert (f["compression"], f["width"], f["height"], f["names"]) == (kind, w, h, names)
        for c in names:
            assert np.array_equal(f["planes"][c], f0["planes"][c]), c
        crypto = sorted(a for a in f0["attrs"] if a.startswith("cryptomatte/"))
        assert len(crypto) == 8 and all(f["attrs"][a] == f0["attrs"][a] for a in crypto)
        assert sorted(set(f["attrs"]) ^ set(f0["attrs"])) == [] and [a for a in f["attrs"] if f["attrs"][a] != f0["attrs"][a]] == ["compression"]
        ygot, ywant = yardstick(raw, 4 * len(names) * w * LINES[kind])
        assert ygot < ywant, "the yardstick does not shrink these chunks: the input proves nothing"
        assert len(data) < len(plain), (len(data), len(plain))
        print(f"{compression}: {len(data)} of {len(plain)} bytes; yardstick chunks {ygot} of {ywant}")
    with pytest.raises(ValueError):
        ctx.write_layers_exr(str(tmp_path / "x.exr"), w, h, fb, compression="piz")
    words_i = ctx.download_ids(bi, w, h)
    check_crypto_layer(pkg, f, "CryptoObject", resolve_expected(words_i), [f"instance#{i}" for i in range(int(words_i[..., 0:6][words_i[..., 6:12] != 0].max()) + 1)])


@pytest.mark.gpu
def test_dropin_program_writes_the_compressed_layers_file(pkg, ctx, manifest, golden_blob, tmp_path):
    """c-ray-hip with CRAY_HIP_EXR=1 CRAY_HIP_EXR_COMPRESSION=zip: the layers file is, byte for byte, what Context.write_layers_exr(compression="zip") writes from
    the same buffers and names; every other file of the run equals the run without the variable."""
    import json
    if not dropin_paths()[2]:
        pytest.skip("c-ray-hip or the asset overlay is not built (needs the reference's sources at build time)")
    m = manifest["cfg1_scene"]
    w, h, s = m["width"], m["height"], m["samples"]
    env = dict(dropin_env(), CRAY_HIP_IDS="4", CRAY_HIP_EXR="1")
    plain, _ = run_dropin(manifest, str(tmp_path / "plain"), env)
    files, text = run_dropin(manifest, str(tmp_path / "zip"), dict(env, CRAY_HIP_EXR_COMPRESSION="zip"))
    assert sorted(files) == sorted(plain)
    for name, data in plain.items():
        assert name == "refrun_layers_0000.exr" or files[name] == data, f"{name} changed"
    data = files["refrun_layers_0000.exr"]
    f, f0 = read_exr(data), read_exr(plain["refrun_layers_0000.exr"])
    assert f["compression"] == 3 and f0["compression"] == 0 and len(data) < len(plain["refrun_layers_0000.exr"])
    for c in f0["names"]:
        assert np.array_equal(f["planes"][c], f0["planes"][c]), c
    inst = list(json.loads(f["attrs"]["cryptomatte/3ae39a5/manifest"][1].decode()))
    mat = list(json.loads(f["attrs"]["cryptomatte/be359d6/manifest"][1].decode()))
    frame = np.frombuffer(files["frame.f32"], np.uint32).reshape(h, w, 3)
    guides = np.frombuffer(files["aov.f32"], np.uint32).reshape(h, w, 8)
    denoised = np.frombuffer(files["denoised.f32"], np.uint32).reshape(h, w, 3)
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    bi, bm = ctx.ids_buffer(w, h), ctx.ids_buffer(w, h)
    ctx.render_ids(bi, bm, w, h, s, pass_count=min(4, s))
    dev = [DeviceArray(pkg, a, np.uint32) for a in (frame, guides, denoised)]
    path = str(tmp_path / "api.exr")
    ctx.write_layers_exr(path, w, h, dev[0].ptr, aov=dev[1].ptr, denoised=dev[2].ptr, instance_ids=bi, material_ids=bm, instance_names=inst, material_names=mat,
                         compression="zip")
    assert open(path, "rb").read() == data


# ---- the CPU tier's run of the above ------------------------------------------------------------------------------------------------------
def test_zip_kernels_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the emulation builds — tests/emu/libcray_hip_exr_emu.so (Makefile.exr: exr_zip.hip unmodified
    on the HIP-on-CPU shim) beside tests/emu/libcray_hip_emu.so, both in one process — every one of them runs and passes there, none skipped (the drop-in test
    where the drop-in program is built)."""
    run_gpu_tests_on_emulation(__file__, 10, passed_without_dropin=9, extra_env={"CRX_LIB": os.path.join(EMU_DIR, "libcray_hip_exr_emu.so")},
                               make_targets=("libcray_hip_emu.so", "-f Makefile.exr"), dropin_libs=("libcray_hip_exr.so",))
