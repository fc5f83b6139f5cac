"""The layers file with 16-bit HALF colour channels: crx_pack of the companion library (include/cray_hip_exr.h, c-ray_amd/csrc/exr_zip.h) packs rows whose channels
are FLOAT or HALF — uncompressed, ZIPS or ZIP —, exr.py and exr_write.c write the typed channel list around the chunks, Context.write_layers_exr(half=...) and the
drop-in program's CRAY_HIP_EXR_HALF=1 choose the colour layers.

The reader (tests/exr_reader.py: mixed HALF / FLOAT planes, compression 0, 2 and 3) is anchored here by a 3 x 1 file spelled out field by field. CPU tier: the
format, the Python writer, the C writer against it under AddressSanitizer and UBSan, the conversion over all 2^32 words against the CPU's F16C instruction, and this
file's GPU tests run by a child pytest on the emulation. GPU tier: the identities with crx_pack_zip and pack_scanlines, every chunk inflated against a numpy
restatement, the conversion on the device, determinism, refusals, a rendered file, the drop-in program."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from exr_reader import (ALL_38, BYTES, F, H, LINES, check_crypto_layer, flat_source, hand_built_2x1, host_chunks, inflate_chunk, read_exr, run_dropin, split_chunks, strip_headers, to_half,
                        typed_rows, zip_case)
from firsthit_spec import resolve_expected
from support import EMU_DIR, REPO, DeviceArray, ctx, dropin_env, dropin_paths, run_gpu_tests_on_emulation  # noqa: F401 (ctx: the fixture)

# the table of the interface (include/cray_hip_exr.h): binary32 word -> binary16 word
TABLE = [(0x7F800001, 0x7C01), (0x7F802000, 0x7C01), (0x7FC00000, 0x7E00), (0x477FEFFF, 0x7BFF), (0x477FF000, 0x7C00), (0x33000000, 0x0000), (0x33000001, 0x0001),
         (0x387FC000, 0x03FF), (0x3F801000, 0x3C00), (0x3F803000, 0x3C02)]


def hand_built_3x1():
    """A 3 x 1 uncompressed image: A FLOAT = (0.25, -0.0, NaN 0x7fc00123), B HALF = (1.0, 65504, -2^-24), C HALF = (+inf, NaN 0x7e00, 0.333251953125)."""
    def attr(name, kind, value):
        return name + b"\0" + kind + b"\0" + struct.pack("<i", len(value)) + value

    def channel(name, pixel_type):
        return name + b"\0" + struct.pack("<i", pixel_type) + struct.pack("<B", 0) + b"\0\0\0" + struct.pack("<i", 1) + struct.pack("<i", 1)
    head = bytes([0x76, 0x2F, 0x31, 0x01]) + bytes([0x02, 0x00, 0x00, 0x00])
    head += attr(b"channels", b"chlist", channel(b"A", 2) + channel(b"B", 1) + channel(b"C", 1) + b"\0")
    head += attr(b"compression", b"compression", struct.pack("<B", 0))
    head += attr(b"dataWindow", b"box2i", struct.pack("<4i", 0, 0, 2, 0))
    head += attr(b"displayWindow", b"box2i", struct.pack("<4i", 0, 0, 2, 0))
    head += attr(b"lineOrder", b"lineOrder", struct.pack("<B", 0))
    head += attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
    head += attr(b"screenWindowCenter", b"v2f", struct.pack("<2f", 0.0, 0.0))
    head += attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0))
    head += b"\0"
    table = struct.pack("<Q", len(head) + 8)
    chunk = struct.pack("<i", 0) + struct.pack("<i", 3 * 4 + 3 * 2 + 3 * 2)
    chunk += struct.pack("<3I", 0x3E800000, 0x80000000, 0x7FC00123)          # A, 4 bytes a pixel
    chunk += struct.pack("<3H", 0x3C00, 0x7BFF, 0x8001)                      # B, 2 bytes a pixel
    chunk += struct.pack("<3H", 0x7C00, 0x7E00, 0x3555)                      # C
    return head + table + chunk


HAND_PLANES = [np.array([[0x3E800000, 0x80000000, 0x7FC00123]], np.uint32),                       # A as it is
               np.array([[0x3F800000, 0x477FE000, 0xB3800000]], np.uint32),                       # B: 1.0, 65504.0, -2^-24 as binary32
               np.array([[0x7F800000, 0x7FC00000, 0x3EAAAAAB]], np.uint32)]                       # C: inf, NaN, 1 / 3 (rounds to 0x3555)
FLAT_PLANES = [np.array([[0x3E800000, 0x80000000]], np.uint32), np.array([[0x3FC00000, 0x7FC00123]], np.uint32)]          # exr_reader.hand_built_2x1's B and R


# ---- CPU tier: the format ---------------------------------------------------------------------------------------------------------------
def test_reader_is_anchored_and_exr_py_writes_the_typed_file(pkg):
    exr = pkg.exr
    data = hand_built_3x1()
    f = read_exr(data)
    assert (f["width"], f["height"], f["names"], f["compression"]) == (3, 1, ["A", "B", "C"], 0) and f["types"] == {"A": F, "B": H, "C": H}
    assert f["planes"]["A"].tolist() == [[0x3E800000, 0x80000000, 0x7FC00123]] and f["planes"]["A"].dtype == np.uint32
    assert f["planes"]["B"].tolist() == [[0x3C00, 0x7BFF, 0x8001]] and f["planes"]["C"].tolist() == [[0x7C00, 0x7E00, 0x3555]] and f["planes"]["C"].dtype == np.uint16
    types = [F, H, H]
    blocks = exr.pack_host(HAND_PLANES, 3, 1, types)
    assert blocks == data[-32:]
    assert exr.file_bytes(3, 1, ["A", "B", "C"], blocks, [32], compression=0, pixel_types=types) == data
    assert exr.header(3, 1, ["A", "B", "C"], pixel_types=types) == data[:-8 - 32]
    # pixel_types=None: today's bytes, from every function
    names, strings = ["A", "B", "C"], {"zzz": "ä"}
    assert exr.header(3, 1, names, strings, 2, None) == exr.header(3, 1, names, strings, 2) == exr.header(3, 1, names, strings, 2, [F, F, F])
    assert exr.header(3, 1, names) == exr.header(3, 1, names, pixel_types=None)
    assert exr.pack_host(HAND_PLANES, 3, 1, None) == exr.pack_host(HAND_PLANES, 3, 1)
    assert exr.pack_host(HAND_PLANES, 3, 1, [F, F, F]) == exr.pack_host(HAND_PLANES, 3, 1), "the typed form of all FLOAT is the packer's layout"
    rng = np.random.default_rng(5)
    planes = [np.repeat(rng.integers(0x3C000000, 0x40000000, (17, 5), dtype=np.uint32), 8, axis=1) for _ in range(3)]
    for kind in (2, 3):
        chunks, sizes = host_chunks(planes, 40, 17, kind, [F, F, F])
        assert exr.file_bytes(40, 17, names, chunks, sizes, strings, kind, None) == exr.file_bytes(40, 17, names, chunks, sizes, strings, kind)
    # compression 0 without types is the flat file, whether its chunks' sizes are stated or not
    flat = exr.pack_host(FLAT_PLANES, 2, 1)
    assert exr.file_bytes(2, 1, ["B", "R"], flat, [24], None, 0) == exr.file_bytes(2, 1, ["B", "R"], flat) == hand_built_2x1()
    with pytest.raises(AssertionError):
        exr.header(3, 1, names, pixel_types=[F, 2, H])
    with pytest.raises(AssertionError):
        exr.header(3, 1, names, pixel_types=[F, H])
    # mixed files of every compression parse to the conversions: deflated chunks, a short last chunk, a chunk of n = 2 (mod 4) bytes
    types = [H, F, H]
    for w in (40, 3):
        planes = [np.repeat(rng.integers(0x3C000000, 0x40000000, (17, -(-w // 8)), dtype=np.uint32), 8, axis=1)[:, :w] for _ in range(3)]
        for kind in (0, 2, 3):
            chunks, sizes = host_chunks(planes, w, 17, kind, types)
            g = read_exr(exr.file_bytes(w, 17, names, chunks, sizes, strings, kind, types))
            assert g["compression"] == kind and len(g["chunks"]) == (2 if kind == 3 else 17) and g["types"] == dict(zip(names, types))
            assert w == 3 or kind == 0 or any(size < n for _, size, n in g["chunks"])
            for name, p, t in zip(names, planes, types):
                assert np.array_equal(g["planes"][name], to_half(p) if t == H else p), (w, kind, name)
            assert g["attrs"]["zzz"] == ("string", "ä".encode())
    # a chunk of n = 2 (mod 4) bytes: 3 FLOAT and 3 HALF pixels
    chunks, sizes = host_chunks(HAND_PLANES[:2], 3, 1, 2, [F, H])
    assert sizes == [8 + 18] and read_exr(exr.file_bytes(3, 1, ["A", "B"], chunks, sizes, None, 2, [F, H]))["planes"]["B"].tolist() == [[0x3C00, 0x7BFF, 0x8001]]
    # the names write_layers_exr(half=...) takes
    lay = sorted(ALL_38, key=lambda s: s.encode())
    t = exr.half_types(lay, True)
    assert [n for n, v in zip(lay, t) if v == H] == sorted(["R", "G", "B", "albedo.R", "albedo.G", "albedo.B", "normal.X", "normal.Y", "normal.Z", "denoised.R", "denoised.G",
                                                              "denoised.B"], key=lambda s: s.encode())
    assert exr.half_types(["B", "G", "R"], True) == [H, H, H] and exr.half_types(lay, ("Z",)) == [H if n == "Z" else F for n in lay]
    for bad in (("nope",), ("CryptoObject00.R",), ("R", "CryptoMaterial02.A")):
        with pytest.raises(ValueError):
            exr.half_types(lay, bad)


C_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "exr_write.h"
/* argv: out width height compression chunk-file size... — the chunks come from the file, their sizes from the command line; the channels are every layer's */
int main(int argc, char **argv) {
	static float dummy[16];
	static uint32_t map[1] = {1};
	crh_pack_channel channels[CRH_PACK_MAX_CHANNELS];
	const char *names[CRH_PACK_MAX_CHANNELS];
	uint8_t types[CRH_PACK_MAX_CHANNELS], bad[CRH_PACK_MAX_CHANNELS];
	/* the 2 x 1 image B = (0.25, -0.0), R = (1.5, a NaN) as one raw chunk: written to <out>.flat with compression 0 and no types */
	static const char *flatNames[2] = {"B", "R"};
	static const uint32_t flat[6] = {0u, 16u, 0x3e800000u, 0x80000000u, 0x3fc00000u, 0x7fc00123u};
	const uint64_t flatSize = sizeof(flat);
	char flatPath[4096];
	struct exr_attr strings[2] = {{"aaa", ""}, {"zzz", "\303\244 \"q\""}};
	if (argc < 7) return 1;
	const int n = exr_layer_channels(dummy, dummy, dummy, dummy, dummy, map, 1, map, 1, channels, names);
	if (n != 38 || exr_half_types(names, n, types) != 12) return 5;
	for (int c = 0; c < n; ++c) bad[c] = types[c];
	bad[n - 1] = 2;
	const int w = atoi(argv[2]), h = atoi(argv[3]), kind = atoi(argv[4]), count = argc - 6;
	uint64_t *sizes = malloc((size_t)count * sizeof(*sizes));
	uint64_t total = 0;
	for (int k = 0; k < count; ++k) { sizes[k] = strtoull(argv[6 + k], NULL, 10); total += sizes[k]; }
	unsigned char *data = malloc(total ? total : 1);
	FILE *f = fopen(argv[5], "rb");
	if (!f || fread(data, 1, total, f) != total) return 3;
	fclose(f);
	const int rc = exr_write_file(argv[1], w, h, names, types, n, strings, 2, kind, data, sizes, count);
	const int refused = exr_write_file(argv[1], w, h, names, types, n, strings, 2, kind, data, sizes, count - 1) == 0 ||
	                    exr_write_file(argv[1], w, h, names, types, n, strings, 2, 1, data, sizes, count) == 0 ||
	                    exr_write_file(argv[1], w, h, names, bad, n, strings, 2, kind, data, sizes, count) == 0;
	snprintf(flatPath, sizeof(flatPath), "%s.flat", argv[1]);
	const int flatRc = exr_write_file(flatPath, 2, 1, flatNames, NULL, 2, NULL, 0, 0, flat, &flatSize, 1);
	for (int c = 0; c < n; ++c) printf("%s %d\n", names[c], types[c]);
	free(sizes); free(data);
	return rc ? 2 : refused ? 4 : flatRc ? 6 : 0;
}
"""


def test_c_typed_writer_writes_the_bytes_of_exr_py(pkg, tmp_path):
    """exr_write_file and exr_half_types in a program of their own (AddressSanitizer and UBSan) against exr.file_bytes(pixel_types=...), byte
    for byte: every layer's 38 channels with the default half set, compression 0, 2 and 3, host-made chunks, a short last chunk; a wrong chunk count, compression 1
    and a pixel type 2 are refused; compression 0 without types writes the flat file, exr.file_bytes' and the hand-built one's bytes."""
    exr = pkg.exr
    host = os.path.join(REPO, "c-ray_amd", "host")
    src, exe = tmp_path / "hc.c", tmp_path / "hc"
    src.write_text(C_PROGRAM)
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(REPO, "include"), "-I" + host, str(src), os.path.join(host, "exr_write.c"), "-o", str(exe)])
    rng = np.random.default_rng(9)
    w, h = 7, 35
    names = sorted(ALL_38, key=lambda s: s.encode())
    types = exr.half_types(names, True)
    planes = [np.repeat(rng.integers(0x3C000000, 0x40000000, (h, 1), dtype=np.uint32), w, axis=1) for _ in names]
    for p in planes:
        p[16:32] = rng.integers(0, 2 ** 32, (16, w), dtype=np.uint32)
    for kind in (0, 2, 3):
        chunks, sizes = host_chunks(planes, w, h, kind, types)
        blob, out = tmp_path / f"chunks{kind}", tmp_path / f"c{kind}.exr"
        blob.write_bytes(chunks)
        r = subprocess.run([str(exe), str(out), str(w), str(h), str(kind), str(blob)] + [str(s) for s in sizes], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert [line.split() for line in r.stdout.splitlines()] == [[n, str(t)] for n, t in zip(names, types)], "exr_half_types chooses what exr.half_types chooses"
        want = exr.file_bytes(w, h, names, chunks, sizes, {"aaa": "", "zzz": "ä \"q\""}, kind, types)
        got = out.read_bytes()
        assert got == want
        assert (tmp_path / f"c{kind}.exr.flat").read_bytes() == exr.file_bytes(2, 1, ["B", "R"], exr.pack_host(FLAT_PLANES, 2, 1)) == hand_built_2x1()
        f = read_exr(got)
        assert kind == 0 or min(sizes) < max(sizes), "deflated chunks among the others"
        for name, p, t in zip(names, planes, types):
            assert np.array_equal(f["planes"][name], to_half(p) if t == H else p), name


# ---- CPU tier: the conversion -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def half_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("half") / "half_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-fopenmp", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           os.path.join(REPO, "tests", "emu", "half_check.cpp"), "-o", exe])
    return exe


def test_conversion_of_every_word_matches_f16c(half_check):
    """exr_zip.h's zipHalfBits, the function the kernels call, over all 2^32 words (tests/emu/half_check.cpp, UBSan, at most 16 threads): the non-NaN ones against
    the CPU's own conversion (_cvtss_sh, round to nearest), the NaNs against the interface's rule stated a second time there."""
    if "f16c" not in open("/proc/cpuinfo").read():
        pytest.skip("this CPU has no F16C: nothing to compare the conversion with")
    out = subprocess.run([half_check], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    text = out.stdout.decode()
    assert out.returncode == 0 and text.startswith("half tested 4294967296 (NaNs 16777214) mismatches 0"), text


def test_conversion_table_and_random_words_match_numpy(half_check, pkg, tmp_path):
    """The interface's table, the edges around it and 400 000 random words: zipHalfBits == numpy's astype(float16) == exr.half_bits."""
    rng = np.random.default_rng(16)
    words = np.concatenate([np.array([w for w, _ in TABLE], np.uint32), np.array([w | 0x80000000 for w, _ in TABLE], np.uint32),
                            np.array([0, 0x80000000, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x32FFFFFF, 0x38800000, 0x387FFFFF,
                                      0x387FE000, 0x387FF000, 0x477FE000, 0x47800000], np.uint32),
                            rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32),
                            rng.integers(0x33000000, 0x47800000, 200000, dtype=np.uint64).astype(np.uint32)])          # (where halves are finite and not zero)
    assert to_half(np.array([w for w, _ in TABLE], np.uint32)).tolist() == [h for _, h in TABLE], "numpy gives the interface's table"
    src, dst = tmp_path / "words", tmp_path / "halves"
    src.write_bytes(words.astype("<u4").tobytes())
    subprocess.check_call([half_check, str(src), str(dst)])
    got = np.frombuffer(dst.read_bytes(), "<u2")
    want = to_half(words)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(words[i]), hex(got[i]), hex(want[i])) for i in bad[:5]]
    assert np.array_equal(pkg.exr.half_bits(words), want)


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


def mixed_case(w, h, types, seed=0):
    """(w, h, sources, channels [(key, stride, component, map key or None)], maps, types): sources of strides 1, 3, 8 and 12; a HALF channel reads ordinary values
    in runs, the packer's special words or random words in turn, every second FLOAT channel is an id channel through a map"""
    rng = np.random.default_rng(1000 * w + 10 * h + len(types) + seed)
    _, _, src, _, maps = zip_case(f"{w}x{h}x1")
    ordinary = (rng.random((h, -(-w // 4), 1), dtype=np.float32) * np.float32(4.0) - np.float32(1.0)).repeat(4, axis=1)[:, :w, :]
    ordinary[rng.random((h, w, 1)) < 0.05] = np.float32(70000.0)          # (above the largest half)
    src["o1"] = np.ascontiguousarray(ordinary).view(np.uint32)
    src["f8"] = flat_source(rng, w, h, 8)
    plain = [("o1", 1, 0, None), ("f3", 3, 0, None), ("f12", 12, 1, None), ("o1", 1, 0, None), ("f8", 8, 5, None), ("f3", 3, 2, None), ("r8", 8, 7, None), ("f12", 12, 11, None)]
    mapped = [("f12", 12, 4, "five"), ("r8", 8, 2, "big")]
    chans, nh, nf = [], 0, 0
    for t in types:
        if t == H:
            chans.append(plain[nh % len(plain)]); nh += 1
        else:
            chans.append(mapped[(nf // 2) % 2] if nf % 2 == 0 else plain[(nf + 3) % len(plain)]); nf += 1
    return w, h, src, chans, maps, list(types)


def run_pack(pkg, ctx, zctx, case, kind, **rows):
    """(crx_pack's bytes, its sizes, the raw bytes expected for the same rows: FLOAT planes from Context.pack_scanlines' words, HALF planes numpy's conversion)"""
    w, h, src, chans, maps, types = case
    dev = {k: DeviceArray(pkg, v, np.uint32) for k, v in src.items()}
    ch = [(dev[k].ptr, stride, comp, None if m is None else maps[m]) for k, stride, comp, m in chans]
    ctx.synchronize()
    data, sizes = zctx.pack(ch, w, h, kind, types, **rows)
    words = np.frombuffer(strip_headers(ctx.pack_scanlines(ch, w, h, **rows), len(chans), w), "<u4").reshape(-1, len(chans), w)
    for c, (k, stride, comp, m) in enumerate(chans):          # (the packer against the sources themselves, where there is no map)
        if m is None:
            first = rows.get("first_row", 0)
            assert np.array_equal(words[:, c], src[k][first:first + words.shape[0], :, comp])
    for k, d in dev.items():
        assert np.array_equal(d.read(ctx), src[k]), "a source was written"
    return data, sizes, typed_rows(words, types).tobytes()


def pattern(floats, halves):
    """`halves` HALF and `floats` FLOAT channels, HALF first and — with two or more — last, the others in turn"""
    inner = [H] * max(halves - 2, 0)
    rest, out = [F] * floats, [H]
    while inner or rest:
        if rest:
            out.append(rest.pop())
        if inner:
            out.append(inner.pop())
    return out + ([H] if halves >= 2 else [])


def one_row_shapes():
    """(w, types) whose row is S - 2, S, S + 2, 2 S - 2, 2 S + 2 bytes"""
    s, out = seg(), []
    for want in (s - 2, s, s + 2, 2 * s - 2, 2 * s + 2):
        found = [(w, pattern((want // w - 2 * halves) // 4, halves)) for w in range(700, 0, -1) if want % w == 0
                 for halves in range(1, 65) if want // w >= 2 * halves and (want // w - 2 * halves) % 4 == 0 and (want // w - 2 * halves) // 4 + halves <= 64]
        assert found and found[0][0] * sum(BYTES[t] for t in found[0][1]) == want, want
        out.append(found[0])
    return out


def layer_types(pkg):
    names = sorted(ALL_38, key=lambda s: s.encode())
    return pkg.exr.half_types(names, True)


@pytest.mark.gpu
def test_all_float_calls_are_the_existing_packers(pkg, ctx, zctx):
    """crx_pack with NULL types and with all-zero types: compression 2 / 3 gives crx_pack_zip's bytes and sizes with 1 / 16 lines, compression 0 gives
    Context.pack_scanlines' bytes."""
    for name in ("3x2x7", "40x17x5", "161x75x38"):
        w, h, src, chans, maps = zip_case(name)
        dev = {k: DeviceArray(pkg, v, np.uint32) for k, v in src.items()}
        ch = [(dev[k].ptr, stride, comp, None if m is None else maps[m]) for k, stride, comp, m in chans]
        ctx.synchronize()
        for kind in (2, 3):
            want, want_sizes = zctx.pack_zip(ch, w, h, LINES[kind])
            for types in (None, [F] * len(ch)):
                data, sizes = zctx.pack(ch, w, h, kind, types)
                assert data == want and np.array_equal(sizes, want_sizes), (name, kind, types)
        blocks = ctx.pack_scanlines(ch, w, h)
        for types in (None, [F] * len(ch)):
            data, sizes = zctx.pack(ch, w, h, 0, types)
            assert data == blocks and sizes.tolist() == [8 + 4 * len(ch) * w] * h, (name, types)
        data, _ = zctx.pack(ch, w, h, 0, None, first_row=1, row_count=h - 1)
        assert data == ctx.pack_scanlines(ch, w, h, 1, h - 1)


@pytest.mark.gpu
def test_mixed_round_trip_against_numpy(pkg, ctx, zctx):
    """Every chunk of compression 0, 2 and 3, inflated and un-transformed, is bit for bit the row layout built on the host: FLOAT planes the packer's words, HALF
    planes numpy's conversion of them. Chunks of n = 2 and n = 2 (mod 4) bytes, ZIP chunks of 16, 1 and 11 lines, a mapped channel between HALF ones, rows of
    S - 2 .. 2 S + 2 bytes; every byte of every chunk is compared."""
    shapes = [(1, 1, [H]), (3, 2, [H, F, H, H]), (5, 17, [F, H]), (67, 5, [H, H, H]), (40, 17, [H, F, F, H, F]), (9, 75, [F, H]), (161, 75, layer_types(pkg))]
    shapes += [(w, 1, types) for w, types in one_row_shapes()]
    assert [w * sum(BYTES[t] for t in types) - seg() for w, h, types in shapes[-5:]] == [-2, 0, 2, seg() - 2, seg() + 2]
    assert (3 * (2 + 4 + 2 + 2)) % 4 == 2, "3 x 2 [H, F, H, H]: n = 2 (mod 4) for ZIPS"
    for w, h, types in shapes:
        case = mixed_case(w, h, types)
        row_bytes = w * sum(BYTES[t] for t in types)
        for kind in (0, 2, 3):
            data, sizes, want = run_pack(pkg, ctx, zctx, case, kind)
            chunks = split_chunks(data, sizes, row_bytes, 0, h, LINES[kind])
            got = b"".join(inflate_chunk(d, n) for _, d, n in chunks)
            assert len(want) == row_bytes * h and len(got) == len(want), (w, h, kind)
            bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
            assert bad.size == 0, (w, h, types, kind, "first wrong byte", int(bad[0]), "row", int(bad[0]) // row_bytes, "at", int(bad[0]) % row_bytes)
            assert int(sizes.sum()) == len(data)
            if kind == 0:
                assert all(len(d) == n for _, d, n in chunks), "compression 0: every chunk raw"
            elif row_bytes >= 240:
                assert any(len(d) < n for _, d, n in chunks), (w, h, kind, "nothing deflated")
            if (w, h) == (1, 1):
                assert len(data) == 10 and data == struct.pack("<ii", 0, 2) + want, "2 bytes come back raw"
            if (w, h, kind) == (40, 17, 3):
                assert [n for _, _, n in chunks] == [row_bytes * 16, row_bytes]
            if (w, h) == (161, 75) and kind == 3:
                assert zctx.time_ms() > 0.0 and len(zctx.phases_ms()) == 4, "the timing entry points report crx_pack"


def conversion_plane():
    """uint32 words: every finite half's exact value, the midpoint to the next half away from zero, the floats one ulp either side of it; the interface's edges,
    NaNs, zeros, float subnormals, FLT_MAX; padded with zeros to a plane of odd width"""
    h16 = np.array([s | m for s in (0, 0x8000) for m in range(0x7C00)], np.uint16)
    assert h16.size == 63488
    value = h16.view(np.float16).astype(np.float64)
    following = np.where((h16 & 0x7FFF) == 0x7BFF, np.copysign(65536.0, value), (h16 + 1).astype(np.uint16).view(np.float16).astype(np.float64))
    mid = ((value + following) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (value + following) / 2), "a midpoint of two halves is a float"
    away = np.nextafter(mid, np.copysign(np.float32(np.inf), mid))
    toward = np.nextafter(mid, np.float32(0.0) * mid)
    exact = value.astype(np.float32)
    assert np.array_equal(to_half(exact.view(np.uint32)), h16), "numpy converts a half's value back to the half"
    edges = np.array([w for w, _ in TABLE] + [w | 0x80000000 for w, _ in TABLE] +
                     [0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFC12345,
                      0x7F801FFF, 0x7F803FFF, 0x32FFFFFF, 0xB3000000, 0xB3000001], np.uint32)
    words = np.concatenate([exact.view(np.uint32), mid.view(np.uint32), away.view(np.uint32), toward.view(np.uint32), edges])
    w = 509
    rows = -(-words.size // w)
    plane = np.zeros(rows * w, np.uint32)
    plane[:words.size] = words
    return plane.reshape(rows, w, 1)


@pytest.mark.gpu
def test_conversion_on_the_device_matches_numpy(pkg, ctx, zctx):
    """One HALF channel over conversion_plane() (about 255 000 words, width 509), compression 0 and 3: the stored halves are numpy's, every one."""
    plane = conversion_plane()
    rows, w, _ = plane.shape
    assert 250000 < plane.size < 270000 and w % 2 == 1
    want = to_half(plane[:, :, 0])
    assert ((want & 0x7FFF) > 0x7C00).sum() >= 10 and (want == 0x7C00).sum() > 3 and ((want & 0x7FFF) < 0x0400).sum() > 4000, "infinities, NaNs and subnormals among them"
    dev = DeviceArray(pkg, plane, np.uint32)
    ctx.synchronize()
    for kind in (0, 3):
        data, sizes = zctx.pack([(dev.ptr, 1, 0)], w, rows, kind, [H])
        chunks = split_chunks(data, sizes, 2 * w, 0, rows, LINES[kind])
        got = np.frombuffer(b"".join(inflate_chunk(d, n) for _, d, n in chunks), "<u2").reshape(rows, w)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (kind, len(bad), [(hex(plane[y, x, 0]), hex(got[y, x]), hex(want[y, x])) for y, x in bad[:5]])
    assert np.array_equal(dev.read(ctx), plane)


@pytest.mark.gpu
def test_determinism_and_row_ranges(pkg, ctx, zctx):
    """67 x 75, nine mixed channels: the same call twice gives equal bytes; first_row ranges (0, 16), (16, 32), (48, rest) concatenate to the single call's bytes and
    sizes; a call of another shape in between changes nothing."""
    case = mixed_case(67, 75, [H, F, H, H, F, F, H, F, H])
    w, h, types = case[0], case[1], case[5]
    row_bytes = w * sum(BYTES[t] for t in types)
    other = mixed_case(3, 2, [H, F, H, H])
    for kind in (0, 2, 3):
        whole, sizes, want = run_pack(pkg, ctx, zctx, case, kind)
        again, sizes2, _ = run_pack(pkg, ctx, zctx, case, kind)
        assert whole == again and np.array_equal(sizes, sizes2) and int(sizes.sum()) == len(whole)
        ranges = ((0, 16), (16, 32), (48, h - 48))
        parts = [run_pack(pkg, ctx, zctx, case, kind, first_row=f, row_count=r) for f, r in ranges]
        assert b"".join(p[0] for p in parts) == whole
        assert np.array_equal(np.concatenate([p[1] for p in parts]), sizes)
        for (data, sz, raw), (f, r) in zip(parts, ranges):
            assert b"".join(inflate_chunk(d, n) for _, d, n in split_chunks(data, sz, row_bytes, f, r, LINES[kind])) == raw
        run_pack(pkg, ctx, zctx, other, kind)
        assert run_pack(pkg, ctx, zctx, case, kind)[0] == whole


@pytest.mark.gpu
def test_refused_arguments_leave_everything_untouched(pkg, ctx, zctx):
    """CRH_ERR_INVALID for every refusal of crx_pack's contract; the output, both size outputs and the sources keep what they held; the next valid call works."""
    abi = pkg.abi
    w, h = 40, 35
    rng = np.random.default_rng(3)
    sa, sb = flat_source(rng, w, h, 3), flat_source(rng, w, h, 8)
    a, b = DeviceArray(pkg, sa, np.uint32), DeviceArray(pkg, sb, np.uint32)
    m = np.arange(7, dtype=np.uint32)
    good = [(a.ptr, 3, 1, None, 0), (b.ptr, 8, 7, m.ctypes.data, 7), (a.ptr, 3, 2, None, 0)]
    good_types = [H, F, H]
    out = np.full(8 * h + 4 * 3 * w * h, 0xA5, np.uint8)
    sizes = np.full(h, 0xA5A5A5A5A5A5A5A5, np.uint64)
    total = C.c_uint64(0x5A5A5A5A5A5A5A5A)
    L = zctx.L

    def call(chans=good, types=good_types, count=None, width=w, height=h, first=0, rows=h, kind=3, handle=zctx.h, dst=out.ctypes.data, null_list=False, sz=sizes.ctypes.data,
             tot=C.byref(total)):
        arr = (abi.PackChannel * 66)()
        for k, c in zip(arr, chans):
            k.dev_src, k.stride, k.component, k.map_host, k.map_count = c
        t = None if types is None else (C.c_uint8 * 66)(*types)
        return L.crx_pack(handle, None if null_list else arr, t, len(chans) if count is None else count, width, height, first, rows, kind, dst, sz, tot)
    refused = {
        "NULL context": dict(handle=None), "NULL list": dict(null_list=True), "NULL output": dict(dst=None), "NULL sizes": dict(sz=None), "NULL total": dict(tot=None),
        "NULL source": dict(chans=[good[0], (None, 3, 0, None, 0)], types=[H, F]), "no channels": dict(count=0), "65 channels": dict(chans=[good[0]] * 65, types=[H] * 65),
        "width 0": dict(width=0), "height 0": dict(height=0), "width < 0": dict(width=-w), "height < 0": dict(height=-h),
        "first_row < 0": dict(first=-16, rows=16), "row_count < 0": dict(rows=-1), "rows past the image": dict(first=16, rows=h), "first_row == height": dict(first=h, rows=1, kind=2),
        "component == stride": dict(chans=[(a.ptr, 3, 3, None, 0)], types=[H]), "stride 0": dict(chans=[(a.ptr, 0, 0, None, 0)], types=[H]),
        "stride 65": dict(chans=[(a.ptr, 65, 0, None, 0)], types=[F]),
        "map_count 65537": dict(chans=[good[0], (b.ptr, 8, 7, m.ctypes.data, 65537)], types=[H, F]), "a map with count 0": dict(chans=[(b.ptr, 8, 7, m.ctypes.data, 0)], types=[F]),
        "compression 1": dict(kind=1), "compression 4": dict(kind=4), "compression -1": dict(kind=-1), "compression 16": dict(kind=16),
        "compression 1, all FLOAT": dict(kind=1, types=None),
        "pixel type 2": dict(types=[H, F, 2]), "pixel type 255": dict(types=[255, F, H]), "HALF on a channel with a map": dict(types=[H, H, H]),
        "HALF on a channel with a map, uncompressed": dict(types=[F, H, F], kind=0),
        "first_row off the chunks": dict(first=8, rows=h - 8), "an end off the chunks": dict(first=0, rows=20), "an end off the chunks, from 16": dict(first=16, rows=3),
        "a FLOAT chunk of 2^31 bytes": dict(chans=[good[0]] * 64, types=None, width=(1 << 31) // (4 * 64 * 16), height=16, rows=16),
        "a HALF chunk of 2^31 bytes": dict(chans=[good[0]] * 64, types=[H] * 64, width=(1 << 31) // (2 * 64 * 16), height=16, rows=16),
    }
    for what, kw in refused.items():
        assert call(**kw) == abi.ERR_INVALID, what
        assert b"crx_pack:" in L.crx_last_error(), what
        assert (out == 0xA5).all() and (sizes == 0xA5A5A5A5A5A5A5A5).all() and total.value == 0x5A5A5A5A5A5A5A5A, what
    for first in (0, 16, 32):          # row_count == 0: CRH_OK, nothing written but the total
        assert call(first=first, rows=0) == abi.OK and total.value == 0
        assert (out == 0xA5).all() and (sizes == 0xA5A5A5A5A5A5A5A5).all()
        total.value = 0x5A5A5A5A5A5A5A5A
    assert np.array_equal(a.read(ctx), sa) and np.array_equal(b.read(ctx), sb), "a refused call wrote a source"
    assert call() == abi.OK
    row_bytes = w * (2 + 4 + 2)
    chunks = split_chunks(out[:total.value].tobytes(), sizes[:3], row_bytes, 0, h, 16)
    words = np.frombuffer(strip_headers(ctx.pack_scanlines([(a.ptr, 3, 1), (b.ptr, 8, 7, m), (a.ptr, 3, 2)], w, h), 3, w), "<u4").reshape(h, 3, w)
    assert b"".join(inflate_chunk(d, n) for _, d, n in chunks) == typed_rows(words, good_types).tobytes()
    assert (out[total.value:] == 0xA5).all() and (sizes[3:] == 0xA5A5A5A5A5A5A5A5).all(), "nothing behind the chunks is written"


@pytest.mark.gpu
def test_rendered_layers_file_with_half_channels(pkg, ctx, golden_blob, manifest, tmp_path):
    """cfg1_scene with the frame, the guides, a denoised frame and both ID buffers, written with half=True as "zip" and "none": the channel list's types are the
    documented ones, every HALF plane is the astype(float16) of the FLOAT plane of the file written with half=False, every FLOAT plane is identical, the
    Cryptomatte layer checks out, the file is smaller than its half=False counterpart. half=("Z",), an unknown name and a Cryptomatte name behave as documented."""
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
    names = sorted(ALL_38, key=lambda s: s.encode())
    half_set = {"R", "G", "B", "albedo.R", "albedo.G", "albedo.B", "normal.X", "normal.Y", "normal.Z", "denoised.R", "denoised.G", "denoised.B"}
    plain = {}
    for compression in ("none", "zip"):
        path = str(tmp_path / f"float_{compression}.exr")
        assert ctx.write_layers_exr(path, w, h, fb, compression=compression, half=False, **kw) == names
        plain[compression] = open(path, "rb").read()
        ctx.write_layers_exr(path + ".default", w, h, fb, compression=compression, **kw)
        assert open(path + ".default", "rb").read() == plain[compression], "half=False is the default and today's bytes"
    f0 = read_exr(plain["none"])
    frame = f0["planes"]["R"].view(np.float32)
    with np.errstate(over="ignore"):
        assert (frame.astype(np.float16).astype(np.float32) != frame).any(), "the frame holds values no half represents: the comparison says something"
    words_i = ctx.download_ids(bi, w, h)
    for compression, kind, chunk_rows in (("zip", 3, 40), ("none", 0, 37), ("zip", 3, None)):
        path = str(tmp_path / f"half_{compression}.exr")
        assert ctx.write_layers_exr(path, w, h, fb, compression=compression, chunk_rows=chunk_rows, half=True, **kw) == names
        data = open(path, "rb").read()
        f = read_exr(data)
        assert (f["compression"], f["width"], f["height"], f["names"]) == (kind, w, h, names)
        assert {c for c in names if f["types"][c] == H} == half_set, "R G B, albedo.*, normal.*, denoised.*: HALF; Z, A and the Cryptomatte channels: FLOAT"
        for c in names:
            want = to_half(f0["planes"][c]) if c in half_set else f0["planes"][c]
            assert f["planes"][c].dtype == want.dtype and np.array_equal(f["planes"][c], want), c
        assert sorted(set(f["attrs"]) ^ set(f0["attrs"])) == [] and sorted(a for a in f["attrs"] if f["attrs"][a] != f0["attrs"][a]) == (["channels", "compression"] if kind else ["channels"])
        check_crypto_layer(pkg, f, "CryptoObject", resolve_expected(words_i), [f"instance#{i}" for i in range(int(words_i[..., 0:6][words_i[..., 6:12] != 0].max()) + 1)])
        assert len(data) < len(plain[compression]), (compression, len(data), len(plain[compression]))
        print(f"{compression}: half {len(data)} of {len(plain[compression])} bytes")
    path = str(tmp_path / "z.exr")
    ctx.write_layers_exr(path, w, h, fb, half=("Z",), **kw)
    f = read_exr(open(path, "rb").read())
    assert [c for c in names if f["types"][c] == H] == ["Z"] and np.array_equal(f["planes"]["Z"], to_half(f0["planes"]["Z"])) and np.array_equal(f["planes"]["R"], f0["planes"]["R"])
    for bad in (("nope",), ("CryptoObject00.R",), ("R", "CryptoMaterial01.G")):
        with pytest.raises(ValueError):
            ctx.write_layers_exr(str(tmp_path / "bad.exr"), w, h, fb, half=bad, **kw)
    assert not os.path.exists(str(tmp_path / "bad.exr"))


@pytest.mark.gpu
def test_dropin_program_writes_the_half_layers_file(pkg, ctx, manifest, golden_blob, tmp_path):
    """c-ray-hip with CRAY_HIP_EXR=1 CRAY_HIP_EXR_HALF=1 CRAY_HIP_EXR_COMPRESSION=zip: the layers file is, byte for byte, what
    Context.write_layers_exr(compression="zip", half=True) writes from the same buffers and names; a value other than 1 leaves the file as it is without the
    variable; every other file of the run is unchanged."""
    import json
    if not dropin_paths()[2]:
        pytest.skip("c-ray-hip or the asset overlay is not built (needs the reference's sources at build time)")
    m = manifest["cfg1_scene"]
    w, h, s = m["width"], m["height"], m["samples"]
    env = dict(dropin_env(), CRAY_HIP_IDS="4", CRAY_HIP_EXR="1", CRAY_HIP_EXR_COMPRESSION="zip")
    plain, _ = run_dropin(manifest, str(tmp_path / "plain"), dict(env, CRAY_HIP_EXR_HALF="yes"))
    files, text = run_dropin(manifest, str(tmp_path / "half"), dict(env, CRAY_HIP_EXR_HALF="1"))
    assert sorted(files) == sorted(plain)
    for name, data in plain.items():
        assert name == "refrun_layers_0000.exr" or files[name] == data, f"{name} changed"
    data = files["refrun_layers_0000.exr"]
    f, f0 = read_exr(data), read_exr(plain["refrun_layers_0000.exr"])
    assert f["compression"] == 3 and f0["compression"] == 3 and len(data) < len(plain["refrun_layers_0000.exr"])
    assert sum(t == H for t in f["types"].values()) == 12 and f["types"]["Z"] == F and f["types"]["R"] == H
    for c in f0["names"]:
        assert np.array_equal(f["planes"][c], to_half(f0["planes"][c]) if f["types"][c] == H else f0["planes"][c]), c
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
                         compression="zip", half=True)
    assert open(path, "rb").read() == data


# ---- the CPU tier's run of the above ------------------------------------------------------------------------------------------------------
def test_half_kernels_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the emulation builds (tests/emu/Makefile.exr: exr_zip.hip unmodified on the HIP-on-CPU shim) —
    every one of them runs and passes there, none skipped (the drop-in test where the drop-in program is built)."""
    run_gpu_tests_on_emulation(__file__, 7, passed_without_dropin=6, extra_env={"CRX_LIB": os.path.join(EMU_DIR, "libcray_hip_exr_emu.so")},
                               make_targets=("libcray_hip_emu.so", "-f Makefile.exr"), dropin_libs=("libcray_hip_exr.so",))
