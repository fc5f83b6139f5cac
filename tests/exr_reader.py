"""The tests' own reader of the layers file, written from the format's description (magic, version, attributes, chlist, offset table, blocks) and anchored by a
2 x 1 file spelled out field by field; the layer list, the Cryptomatte checks, the planted edge values and the drop-in run that the uncompressed and the
compressed file's tests share (no test lives here; tests/test_exr_layers.py and tests/test_exr_zip.py use it)."""
import json
import os
import re
import struct

import numpy as np

import support

GUIDES = ("albedo.R", "albedo.G", "albedo.B", "normal.X", "normal.Y", "normal.Z", "Z", "A")


def crypto_names(layer):
    """rank r: id in <layer>0k.R (r = 2k) or .B (r = 2k + 1), coverage in .G or .A"""
    return [(f"{layer}{r // 2:02d}.{'RB'[r % 2]}", f"{layer}{r // 2:02d}.{'GA'[r % 2]}") for r in range(6)]


ALL_38 = ["R", "G", "B"] + list(GUIDES) + ["denoised.R", "denoised.G", "denoised.B"] + [n for layer in ("CryptoObject", "CryptoMaterial") for pair in crypto_names(layer) for n in pair]
assert len(ALL_38) == 38


# ---- the reader ---------------------------------------------------------------------------------------------------------------------------
def _cstr(data, pos):
    end = data.index(b"\0", pos)
    return data[pos:end], end + 1


def read_exr(data):
    """An uncompressed single-part scanline OpenEXR file whose channels are all FLOAT -> width, height, attributes {name: (type, value bytes)} and their order,
    channel names in file order, planes {name: uint32 [H, W]}, the offset table, the y of every block in file order, where the first block starts and the last ends."""
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
    names, at = [], 0
    while chl[at] != 0:
        name, at = _cstr(chl, at)
        pixel_type, p_linear, z0, z1, z2, xs, ys = struct.unpack_from("<iBBBBii", chl, at)
        assert (pixel_type, p_linear, z0, z1, z2, xs, ys) == (2, 0, 0, 0, 0, 1, 1), name
        assert 1 <= len(name) <= 31
        names.append(name.decode())
        at += 16
    assert at == len(chl) - 1
    assert attrs["compression"] == ("compression", b"\0") and attrs["lineOrder"] == ("lineOrder", b"\0")
    assert attrs["dataWindow"][0] == "box2i" and attrs["displayWindow"] == attrs["dataWindow"]
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    assert (x0, y0) == (0, 0)
    w, h = x1 + 1, y1 + 1
    assert attrs["pixelAspectRatio"] == ("float", struct.pack("<f", 1.0)) and attrs["screenWindowWidth"] == ("float", struct.pack("<f", 1.0))
    assert attrs["screenWindowCenter"] == ("v2f", struct.pack("<2f", 0.0, 0.0))
    offsets = list(struct.unpack_from(f"<{h}Q", data, pos))
    pos += 8 * h
    first = pos
    planes = np.empty((len(names), h, w), np.uint32)
    ys = []
    for y in range(h):          # (in file order)
        yy, size = struct.unpack_from("<ii", data, pos)
        assert size == 4 * len(names) * w, "a block's byte count"
        ys.append(yy)
        planes[:, yy, :] = np.frombuffer(data, "<u4", len(names) * w, pos + 8).reshape(len(names), w)
        pos += 8 + size
    return {"width": w, "height": h, "attrs": attrs, "attr_order": order, "names": names, "planes": dict(zip(names, planes)), "offsets": offsets, "ys": ys,
            "first": first, "end": pos}


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
