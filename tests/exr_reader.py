"""The tests' own reader of the layers file, written from the format's description (magic, version, attributes, chlist, offset table, chunks) — FLOAT and HALF
channels, uncompressed, ZIPS or ZIP: it inflates with Python's zlib and undoes the predictor and the byte split — and anchored by three files spelled out field by
field (hand_built_2x1 here, hand_built_2x1_zips in tests/test_exr_zip.py, hand_built_3x1 in tests/test_exr_half.py); OpenEXR's ZIP transform and the chunks of a
pack made on the host; the layer list, the Cryptomatte checks, the packers' sources with their planted edge values and the drop-in run (no test lives here;
tests/test_exr_layers.py, tests/test_exr_zip.py and tests/test_exr_half.py use it)."""
import json
import os
import re
import struct
import zlib

import numpy as np

import support

LINES = {0: 1, 2: 1, 3: 16}          # rows a chunk, by the compression attribute
F, H = 0, 1                          # pixel types as crx_pack takes them; the file's chlist says 2 and 1
BYTES = {F: 4, H: 2}
GUIDES = ("albedo.R", "albedo.G", "albedo.B", "normal.X", "normal.Y", "normal.Z", "Z", "A")


def crypto_names(layer):
    """rank r: id in <layer>0k.R (r = 2k) or .B (r = 2k + 1), coverage in .G or .A"""
    return [(f"{layer}{r // 2:02d}.{'RB'[r % 2]}", f"{layer}{r // 2:02d}.{'GA'[r % 2]}") for r in range(6)]


ALL_38 = ["R", "G", "B"] + list(GUIDES) + ["denoised.R", "denoised.G", "denoised.B"] + [n for layer in ("CryptoObject", "CryptoMaterial") for pair in crypto_names(layer) for n in pair]
assert len(ALL_38) == 38


# ---- OpenEXR's ZIP transform and the conversion to HALF, on the host ------------------------------------------------------------------------
def zip_forward(raw):
    """raw bytes R -> T': even bytes first, then odd ones; then every byte but the first becomes its difference to its predecessor + 128"""
    r = np.frombuffer(bytes(raw), np.uint8)
    t = np.concatenate([r[0::2], r[1::2]]).astype(np.int64)
    p = t.copy()
    p[1:] = (t[1:] - t[:-1] + 128) & 255
    return p.astype(np.uint8).tobytes()


def zip_inverse(tp):
    """T' -> R"""
    p = np.frombuffer(bytes(tp), np.uint8).astype(np.int64)
    n = p.size
    t = ((np.cumsum(p) - 128 * np.arange(n)) & 255).astype(np.uint8)
    r = np.empty(n, np.uint8)
    r[0::2] = t[:(n + 1) // 2]
    r[1::2] = t[(n + 1) // 2:]
    return r.tobytes()


def inflate_chunk(data, n):
    """the raw bytes of a chunk's data (n: its raw size): size == n is raw, anything else a complete zlib stream of T' with nothing behind it"""
    if len(data) == n:
        return bytes(data)
    assert len(data) < n, "a chunk larger than its raw bytes"
    assert data[0:2] == b"\x78\x01", "zlib header: CM 8, 32 K window, no dictionary"
    d = zlib.decompressobj()
    tp = d.decompress(bytes(data))
    assert d.eof and d.unused_data == b"" and len(tp) == n, "one complete zlib stream of n bytes"
    return zip_inverse(tp)


def to_half(words):
    """numpy's conversion of 32-bit words read as binary32: the uint16 bits"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(words, np.uint32).view(np.float32).astype(np.float16).view(np.uint16)


# ---- the reader ---------------------------------------------------------------------------------------------------------------------------
def _cstr(data, pos):
    end = data.index(b"\0", pos)
    return data[pos:end], end + 1


def read_exr(data):
    """A single-part scanline OpenEXR file whose channels are FLOAT or HALF, uncompressed, ZIPS or ZIP -> width, height, attributes {name: (type, value bytes)} and
    their order, channel names in file order, types {name: F or H}, planes {name: uint32 or uint16 [H, W]}, compression, the offset table, chunks [(y, size, n)] and
    their ys in file order, where the first chunk starts and the last ends. Every offset is checked against the position of its chunk."""
    assert data[0:4] == bytes([0x76, 0x2F, 0x31, 0x01]), "magic"
    assert data[4:8] == bytes([2, 0, 0, 0]), "version 2, no flags: single part, scanline, short names"
    pos, attrs, order = 8, {}, []
    while data[pos] != 0:
        name, pos = _cstr(data, pos)
        kind, pos = _cstr(data, pos)
        size, = struct.unpack_from("<i", data, pos)
        assert 1 <= len(name) <= 31 and size >= 0
        attrs[name.decode()] = (kind.decode(), data[pos + 4:pos + 4 + size])
        order.append(name)
        pos += 4 + size
    pos += 1
    kind, chl = attrs["channels"]
    assert kind == "chlist" and chl[-1] == 0
    names, types, at = [], [], 0
    while chl[at] != 0:
        name, at = _cstr(chl, at)
        pixel_type, *rest = struct.unpack_from("<iBBBBii", chl, at)          # pixelType, pLinear, three zero bytes, xSampling, ySampling
        assert pixel_type in (1, 2) and rest == [0, 0, 0, 0, 1, 1], name
        assert 1 <= len(name) <= 31
        names.append(name.decode())
        types.append(H if pixel_type == 1 else F)
        at += 16
    assert at == len(chl) - 1
    kind = attrs["compression"][1][0]
    assert attrs["compression"] == ("compression", bytes([kind])) and kind in (0, 2, 3) and attrs["lineOrder"] == ("lineOrder", b"\0")
    assert attrs["dataWindow"][0] == "box2i" and attrs["displayWindow"] == attrs["dataWindow"]
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    assert (x0, y0) == (0, 0)
    w, h, lines = x1 + 1, y1 + 1, LINES[kind]
    assert attrs["pixelAspectRatio"] == ("float", struct.pack("<f", 1.0)) and attrs["screenWindowWidth"] == ("float", struct.pack("<f", 1.0))
    assert attrs["screenWindowCenter"] == ("v2f", struct.pack("<2f", 0.0, 0.0))
    row_bytes = w * sum(BYTES[t] for t in types)
    count = -(-h // lines)
    offsets = list(struct.unpack_from(f"<{count}Q", data, pos))
    pos += 8 * count
    first = pos
    raw, chunks = [], []
    for k in range(count):          # (in file order)
        assert offsets[k] == pos, "every offset is the position of its chunk"
        y, size = struct.unpack_from("<ii", data, pos)
        n = row_bytes * min(lines, h - k * lines)
        assert y == k * lines and 0 < size <= n and (kind != 0 or size == n), "chunks in row order; a chunk's byte count"
        raw.append(inflate_chunk(data[pos + 8:pos + 8 + size], n))
        chunks.append((y, size, n))
        pos += 8 + size
    assert pos == len(data), "nothing behind the last chunk"
    assert order == sorted(order) and [s.encode() for s in names] == sorted(s.encode() for s in names)
    rows = np.frombuffer(b"".join(raw), np.uint8).reshape(h, row_bytes)
    planes, at = {}, 0
    for name, t in zip(names, types):
        planes[name] = np.ascontiguousarray(rows[:, at:at + BYTES[t] * w]).view("<u2" if t == H else "<u4").astype(np.uint16 if t == H else np.uint32)
        at += BYTES[t] * w
    assert at == row_bytes
    return {"width": w, "height": h, "attrs": attrs, "attr_order": order, "names": names, "types": dict(zip(names, types)), "planes": planes, "offsets": offsets,
            "ys": [c[0] for c in chunks], "first": first, "end": pos, "compression": kind, "chunks": chunks}


def attr_string(f, name):
    kind, value = f["attrs"][name]
    assert kind == "string"
    return value.decode("utf-8")


def hand_built_2x1():
    """A 2 x 1 image with the channels B and R: B = (0.25, -0.0), R = (1.5, NaN 0x7fc00123)."""
    def attr(name, kind, value):
        return name + b"\0" + kind + b"\0" + struct.pack("<i", len(value)) + value

    def channel(name):
        return name + b"\0" + struct.pack("<i", 2) + struct.pack("<B", 0) + b"\0\0\0" + struct.pack("<i", 1) + struct.pack("<i", 1)
    head = bytes([0x76, 0x2F, 0x31, 0x01]) + bytes([0x02, 0x00, 0x00, 0x00])
    head += attr(b"channels", b"chlist", channel(b"B") + channel(b"R") + b"\0")
    head += attr(b"compression", b"compression", struct.pack("<B", 0))
    head += attr(b"dataWindow", b"box2i", struct.pack("<i", 0) + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 0))
    head += attr(b"displayWindow", b"box2i", struct.pack("<i", 0) + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 0))
    head += attr(b"lineOrder", b"lineOrder", struct.pack("<B", 0))
    head += attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
    head += attr(b"screenWindowCenter", b"v2f", struct.pack("<f", 0.0) + struct.pack("<f", 0.0))
    head += attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0))
    head += b"\0"
    table = struct.pack("<Q", len(head) + 8)          # one row: its block follows the one-entry table
    block = struct.pack("<i", 0) + struct.pack("<i", 4 * 2 * 2)
    block += struct.pack("<I", 0x3E800000) + struct.pack("<I", 0x80000000)          # B: 0.25, -0.0
    block += struct.pack("<I", 0x3FC00000) + struct.pack("<I", 0x7FC00123)          # R: 1.5, a NaN with a payload
    return head + table + block


# ---- what goes into the packers -----------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0x7FC00000, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00000000, 0x3F800000], np.uint32)


def plant_ids(rng, a, comp, count):
    """component `comp` of `a` becomes ids against a map of `count` entries: the edge values first, valid ids behind them"""
    edge = np.array([-1.0, 0.0, count - 1, count, 2.5, np.nan, 16777216.0, -0.0, 0.5, count - 0.5, 1e30, np.inf, -np.inf, 1e-45, -2.0, 4294967296.0], np.float32)
    vals = rng.integers(0, count, a.shape[0] * a.shape[1]).astype(np.float32)
    vals[:min(edge.size, vals.size)] = edge[:vals.size]
    a[:, :, comp] = vals.view(np.uint32).reshape(a.shape[:2])


def flat_source(rng, w, h, stride):
    """uint32 [h, w, stride] that deflates: per component runs of a few columns of one word — NaNs with payloads, infinities, -0.0, subnormals among them — with
    a random word every so often"""
    pick = rng.integers(0, SPECIAL.size, (h, -(-w // 5), stride))
    a = np.repeat(SPECIAL[pick], 5, axis=1)[:, :w, :].copy()
    noise = rng.random((h, w, stride)) < 0.03
    a[noise] = rng.integers(0, 2 ** 32, int(noise.sum()), dtype=np.uint32)
    return np.ascontiguousarray(a)


def zip_case(name):
    """(w, h, sources {key: uint32 array}, channels [(key, stride, component, map key or None)], maps) — flat and random sources mixed, ids through maps"""
    rng = np.random.default_rng(sum(name.encode()))
    maps = {"big": rng.integers(0, 2 ** 32, 65536, dtype=np.uint32), "five": rng.integers(1, 2 ** 32, 5, dtype=np.uint32)}
    w, h, nch = (int(v) for v in name.split("x"))
    src = {"f3": flat_source(rng, w, h, 3), "f12": flat_source(rng, w, h, 12), "r8": rng.integers(0, 2 ** 32, (h, w, 8), dtype=np.uint32)}
    ids = (rng.integers(0, 5, (h, -(-w // 7))).repeat(7, axis=1)[:, :w]).astype(np.float32)          # ids in runs, the edge values of plant_ids in front
    src["f12"][:, :, 4] = ids.view(np.uint32)
    edge = np.array([-1.0, 0.0, 4, 5, 2.5, np.nan, 16777216.0, -0.0, 0.5, 4.5, 1e30, np.inf, -np.inf, 1e-45, -2.0, 4294967296.0], np.float32).view(np.uint32)
    flat = src["f12"][:, :, 4].reshape(-1)
    flat[:min(16, flat.size)] = edge[:flat.size]
    src["f12"][:, :, 4] = flat.reshape(h, w)
    plant_ids(rng, src["r8"], 2, 65536)
    pool = [("f3", 3, 0, None), ("f12", 12, 4, "five"), ("f12", 12, 1, None), ("r8", 8, 2, "big"), ("f3", 3, 2, None), ("f12", 12, 11, None), ("r8", 8, 7, None),
            ("f3", 3, 1, None)]
    chans = [pool[i % len(pool)] if i < len(pool) else ("f12", 12, i % 12, None) for i in range(nch)]
    return w, h, src, chans, maps


# ---- what comes out of them -----------------------------------------------------------------------------------------------------------------
def typed_rows(words, types):
    """uint32 [rows, channels, w] -> uint8 [rows, rowBytes]: a plane per channel, 4-byte words or their 2-byte conversions, little-endian"""
    parts = [(to_half(words[:, c]).astype("<u2") if t == H else words[:, c].astype("<u4")).view(np.uint8).reshape(words.shape[0], -1) for c, t in enumerate(types)]
    return np.concatenate(parts, axis=1)


def host_chunks(planes, w, h, kind, types=None):
    """crx_pack's chunks made on the host from [h, w] planes in channel order (types None: all FLOAT, crx_pack_zip's): (data, sizes). Compression 0 leaves
    every chunk raw, and so does 2 / 3 where the stream (zlib level 1: the header is 78 01) is not shorter."""
    rows = typed_rows(np.stack([np.ascontiguousarray(p).view(np.uint32).reshape(h, w) for p in planes], axis=1), [F] * len(planes) if types is None else types)
    data, sizes = b"", []
    for y in range(0, h, LINES[kind]):
        raw = rows[y:y + LINES[kind]].tobytes()
        z = zlib.compress(zip_forward(raw), 1) if kind else raw
        body = z if len(z) < len(raw) else raw
        data += struct.pack("<ii", y, len(body)) + body
        sizes.append(8 + len(body))
    return data, sizes


def split_chunks(data, sizes, row_bytes, first, rows, lines):
    """crx_pack's or crx_pack_zip's output -> [(y, data bytes, n)] after checking the layout: chunks back to back in row order, sizes as stated"""
    out, at = [], 0
    assert len(sizes) == -(-rows // lines)
    for k, total in enumerate(int(v) for v in sizes):
        y, size = struct.unpack_from("<ii", data, at)
        n = row_bytes * min(lines, rows - k * lines)
        assert y == first + k * lines and total == 8 + size and 0 < size <= n, (k, y, size, n)
        out.append((y, data[at + 8:at + 8 + size], n))
        at += total
    assert at == len(data)
    return out


def raw_of(chunks):
    return b"".join(inflate_chunk(d, n) for _, d, n in chunks)


def strip_headers(blocks, nch, w):
    """Context.pack_scanlines' bytes without the 8-byte header of every row"""
    return np.frombuffer(blocks, np.uint8).reshape(-1, 8 + 4 * nch * w)[:, 8:].tobytes()


# ---- the Cryptomatte layers of a file -------------------------------------------------------------------------------------------------------
def check_crypto_layer(pkg, f, layer, ranked, names):
    """The id channels hold the names' converted hashes (0.0f where the rank is empty), the coverage channels the ranked coverages; the manifest inverts."""
    exr = pkg.exr
    manifest = json.loads(attr_string(f, f"cryptomatte/{exr.layer_key(layer)}/manifest"))
    assert list(manifest) == list(names), "keys in id order"
    assert [int(v, 16) for v in manifest.values()] == [exr.crypto_id(s) for s in names] and all(re.fullmatch(r"[0-9a-f]{8}", v) for v in manifest.values())
    index = {int(v, 16): i for i, v in enumerate(manifest.values())}
    assert len(index) == len(names), "the manifest inverts to the indices"
    assert attr_string(f, f"cryptomatte/{exr.layer_key(layer)}/name") == layer
    assert attr_string(f, f"cryptomatte/{exr.layer_key(layer)}/hash") == "MurmurHash3_32"
    assert attr_string(f, f"cryptomatte/{exr.layer_key(layer)}/conversion") == "uint32_to_float32"
    table = np.array([exr.crypto_id(s) for s in names], np.uint32)
    for r, (idn, covn) in enumerate(crypto_names(layer)):
        ids = ranked[..., r, 0]
        empty = ids < 0
        assert (ids[~empty] < len(names)).all()
        want = np.where(empty, np.uint32(0), table[np.where(empty, 0, ids).astype(np.int64)])
        assert np.array_equal(f["planes"][idn], want), idn
        assert np.array_equal(f["planes"][covn], ranked[..., r, 1].view(np.uint32)), covn
        back = np.array([index[int(v)] for v in f["planes"][idn][~empty]], np.float32)
        assert np.array_equal(back, ids[~empty]), "the file's ids invert to the indices through the manifest"


# ---- the drop-in program ------------------------------------------------------------------------------------------------------------------
def run_dropin(manifest, out_dir, extra_env):
    """c-ray-hip on cfg1_scene with CRAY_HIP_AOV=4 CRAY_HIP_DENOISE=2 and `extra_env`: the float dumps of the frame, the guides and the denoised frame among
    every file it wrote ({name: bytes}), and its output."""
    dumps = {var: os.path.join(out_dir, name + ".f32") for var, name in (("CRH_DUMP_F32", "frame"), ("CRH_DUMP_AOV_F32", "aov"), ("CRH_DUMP_DENOISED_F32", "denoised"))}
    return support.run_dropin(manifest, out_dir, dict(dumps, CRAY_HIP_AOV="4", CRAY_HIP_DENOISE="2", **extra_env))
