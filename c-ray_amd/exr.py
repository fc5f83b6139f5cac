"""exr.py — the host side of the multi-layer OpenEXR output: a single-part scanline file whose channels are FLOAT or, where asked for, HALF (`pixel_types`;
Context.write_layers_exr(half=...)), uncompressed, or ZIP / ZIPS compressed from chunks deflated on the device (Context.write_layers_exr(compression=...), exrzip.py), and
Cryptomatte's naming of ids.
The pixel data comes packed from the device (Context.pack_scanlines: crh_pack_scanlines, include/cray_hip.h; ZipContext.pack: crx_pack, include/cray_hip_exr.h); this
module writes what goes around it — header, offset table — and knows which channel of which buffer carries which name. c-ray_amd/host/exr_write.c states the same in C
for the drop-in program; both write the same bytes.

File layout: magic 76 2f 31 01, version 02 00 00 00, attributes in ascending byte order of name (each `name\\0 type\\0 int32 size, value`), one \\0, one uint64 absolute
offset per chunk, then the chunks in row order (row 0 = the top of the image = y 0, lineOrder increasing y): a chunk is int32 y of its first row, int32 byte count and
the data of LINES_PER_CHUNK[compression] rows, the last chunk of the image the rows that are left. A row is one plane of `width` pixels per channel, channels in
ascending byte order of name, 4 bytes a FLOAT pixel and 2 a HALF one. Compression 0: a chunk is a row as it is — crh_pack_scanlines' block; 2 (ZIPS) and 3 (ZIP): the
rows' bytes transformed and deflated, or as they are where that is not shorter (include/cray_hip_exr.h).
"""
import json
import struct

import numpy as np

MAX_NAME = 31          # attribute and channel names of a file whose version field has no long-names bit
CRYPTO_LAYERS = ("CryptoObject", "CryptoMaterial")
CRYPTO_RANKS = 6       # crh_ids_resolve's ranks: three RGBA layers of two (id, coverage) pairs


def murmur3_32(data, seed=0):
    """MurmurHash3_x86_32 of a bytes object."""
    c1, c2, m = 0xCC9E2D51, 0x1B873593, 0xFFFFFFFF
    h = seed & m
    n = len(data)
    for i in range(0, n - n % 4, 4):
        k = struct.unpack_from("<I", data, i)[0]
        k = (k * c1) & m
        k = ((k << 15) | (k >> 17)) & m
        k = (k * c2) & m
        h ^= k
        h = ((h << 13) | (h >> 19)) & m
        h = (h * 5 + 0xE6546B64) & m
    k = 0
    tail = data[n - n % 4:]
    for j in range(len(tail) - 1, -1, -1):
        k = (k << 8) | tail[j]
    if tail:
        k = (k * c1) & m
        k = ((k << 15) | (k >> 17)) & m
        k = (k * c2) & m
        h ^= k
    h ^= n
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m
    h ^= h >> 16
    return h


def float_safe(h):
    """Cryptomatte's uint32_to_float32 conversion: a word whose exponent field is 0 or 255 (a denormal, an infinity, a NaN) gets bit 23 flipped."""
    return h ^ (1 << 23) if ((h >> 23) & 255) in (0, 255) else h


def crypto_id(name):
    """The 32-bit word a Cryptomatte id channel holds for the name."""
    return float_safe(murmur3_32(name.encode("utf-8")))


def layer_key(layer):
    """The <k> of a layer's `cryptomatte/<k>/...` attributes: the first 7 hex digits of its name's id."""
    return ("%08x" % crypto_id(layer))[:7]


def id_map(names):
    """map[i] = crypto_id(names[i]) as the uint32 array crh_pack_scanlines takes; the names must be unique (a manifest maps a name to one id)."""
    names = list(names)
    assert len(set(names)) == len(names), "names of a Cryptomatte layer must be unique"
    return np.array([crypto_id(s) for s in names], dtype=np.uint32)


def manifest(names):
    """name -> 8 lowercase hex digits of its id, keys in id order, no whitespace."""
    return json.dumps({s: "%08x" % crypto_id(s) for s in names}, separators=(",", ":"), ensure_ascii=False)


def crypto_attributes(layer, names):
    k = layer_key(layer)
    return {f"cryptomatte/{k}/name": layer, f"cryptomatte/{k}/hash": "MurmurHash3_32", f"cryptomatte/{k}/conversion": "uint32_to_float32",
            f"cryptomatte/{k}/manifest": manifest(names)}


def crypto_channels(layer):
    """The twelve channel names of a layer in rank order: (id, coverage) of rank 2k in <layer>0k.R / .G, of rank 2k + 1 in .B / .A."""
    return [f"{layer}{r // 2:02d}.{'RGBA'[2 * (r % 2) + part]}" for r in range(CRYPTO_RANKS) for part in (0, 1)]


def _attr(name, kind, value):
    raw = name.encode("utf-8")
    assert 0 < len(raw) <= MAX_NAME, f"attribute name {name!r} is longer than {MAX_NAME} bytes"
    return raw + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(value)) + value


FLOAT, HALF = 0, 1          # pixel types as crx_pack takes them (include/cray_hip_exr.h); the file's chlist says 2 and 1
PIXEL_BYTES = {FLOAT: 4, HALF: 2}


def header(width, height, channel_names, strings=None, compression=0, pixel_types=None):
    """The bytes before the offset table. channel_names must be in ascending byte order; `strings` are further attributes of type string; `compression` is the
    value of the attribute of that name: 0 none, 2 ZIPS (a chunk a row), 3 ZIP (a chunk every 16 rows); `pixel_types`: FLOAT or HALF per channel (None: all FLOAT)."""
    assert compression in (0, 2, 3)
    types = [FLOAT] * len(channel_names) if pixel_types is None else [int(t) for t in pixel_types]
    assert len(types) == len(channel_names) and all(t in PIXEL_BYTES for t in types), "one pixel type, FLOAT or HALF, per channel"
    raw = [c.encode("utf-8") for c in channel_names]
    assert raw == sorted(raw) and len(set(raw)) == len(raw), "channels must be unique and in ascending byte order of name"
    chlist = b""
    for c, t in zip(raw, types):
        assert 0 < len(c) <= MAX_NAME, f"channel name {c!r} is longer than {MAX_NAME} bytes"
        chlist += c + b"\0" + struct.pack("<iB3xii", 1 if t == HALF else 2, 0, 1, 1)          # HALF 1 / FLOAT 2, pLinear 0, xSampling 1, ySampling 1
    chlist += b"\0"
    window = struct.pack("<4i", 0, 0, width - 1, height - 1)
    attrs = {"channels": ("chlist", chlist), "compression": ("compression", bytes([compression])), "dataWindow": ("box2i", window), "displayWindow": ("box2i", window),
             "lineOrder": ("lineOrder", b"\0"), "pixelAspectRatio": ("float", struct.pack("<f", 1.0)), "screenWindowCenter": ("v2f", struct.pack("<2f", 0.0, 0.0)),
             "screenWindowWidth": ("float", struct.pack("<f", 1.0))}
    for k, v in (strings or {}).items():
        assert k not in attrs
        attrs[k] = ("string", v.encode("utf-8"))
    out = bytes([0x76, 0x2F, 0x31, 0x01, 2, 0, 0, 0])
    for k in sorted(attrs, key=lambda s: s.encode("utf-8")):
        out += _attr(k, *attrs[k])
    return out + b"\0"


LINES_PER_CHUNK = {0: 1, 2: 1, 3: 16}          # by the compression attribute


def file_bytes(width, height, channel_names, chunk_data, chunk_sizes=None, strings=None, compression=0, pixel_types=None):
    """The whole file: `chunk_data` is the chunks back to back in row order as crx_pack writes them (include/cray_hip_exr.h: int32 y, int32 size, `size` bytes),
    `chunk_sizes` their byte counts (8 + size). The offset table has one entry per chunk; the chunks follow verbatim. chunk_sizes None, for compression 0 only: every
    chunk is a row of 8 + rowBytes bytes, which is what Context.pack_scanlines and pack_host return."""
    head = header(width, height, channel_names, strings, compression, pixel_types)
    if chunk_sizes is None:
        assert compression == 0, "only the chunks of an uncompressed file have a size that follows from the header"
        chunk_sizes = [8 + width * sum(PIXEL_BYTES[int(t)] for t in (pixel_types if pixel_types is not None else [FLOAT] * len(channel_names)))] * height
    sizes = [int(v) for v in chunk_sizes]
    assert len(sizes) == -(-height // LINES_PER_CHUNK[compression]), "one chunk for every LINES_PER_CHUNK rows"
    assert sum(sizes) == len(chunk_data) and all(v >= 8 for v in sizes), "the chunk sizes do not add up to the chunk data"
    at, offsets = len(head) + 8 * len(sizes), []
    for v in sizes:
        offsets.append(at)
        at += v
    return head + struct.pack(f"<{len(sizes)}Q", *offsets) + bytes(chunk_data)


def half_bits(words):
    """The binary16 bits crx_pack stores for 32-bit words read as binary32 (include/cray_hip_exr.h's rule: numpy's astype(float16))."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(words).view(np.float32).astype(np.float16).view(np.uint16)


def pack_host(planes, width, height, pixel_types=None):
    """The pixel data from host arrays — planes: [height, width] arrays of 32-bit words in channel order —, for files that never were on a device, as crx_pack lays
    out compression 0: per row int32 y, int32 rowBytes and a plane per channel of 4-byte words or, for HALF, of the words' binary16 conversions. `pixel_types` None:
    all FLOAT, crh_pack_scanlines' blocks. file_bytes(..., pixel_types=pixel_types) takes it."""
    types = [FLOAT] * len(planes) if pixel_types is None else pixel_types
    assert len(types) == len(planes)
    words = [np.ascontiguousarray(p).view(np.uint32).reshape(height, width) for p in planes]
    typed = [half_bits(p).astype("<u2").view(np.uint8) if t == HALF else p.astype("<u4").view(np.uint8) for p, t in zip(words, types)]
    head = np.empty((height, 2), "<u4")
    head[:, 0], head[:, 1] = np.arange(height), width * sum(PIXEL_BYTES[t] for t in types)
    return np.concatenate([head.view(np.uint8).reshape(height, 8)] + [t.reshape(height, -1) for t in typed], axis=1).tobytes()


HALF_DEFAULT = ("R", "G", "B", "albedo.R", "albedo.G", "albedo.B", "normal.X", "normal.Y", "normal.Z", "denoised.R", "denoised.G", "denoised.B")


def half_types(names, half):
    """The pixel type of every channel of `names` for write_layers_exr's `half`: True is HALF_DEFAULT — the colour-like layers; Z, A and the Cryptomatte channels stay
    FLOAT —, an iterable of channel names exactly those. ValueError for a name that is not in the file or a Cryptomatte channel (an id is a 32-bit word, and a
    matte's coverages stay beside it). Values above 65504 become infinity in a HALF channel: that is the format."""
    if isinstance(half, (bool, int)):
        chosen = set(HALF_DEFAULT) & set(names)
    else:
        chosen = {half} if isinstance(half, str) else set(half)
        for n in sorted(chosen):
            if n not in names:
                raise ValueError(f"half: the file has no channel {n!r}")
            if n.startswith(CRYPTO_LAYERS):
                raise ValueError(f"half: {n!r} is a Cryptomatte channel and stays FLOAT")
    return [HALF if n in chosen else FLOAT for n in names]


def layer_channels(fb, aov=None, denoised=None, instance_ranked=None, material_ranked=None, instance_map=None, material_map=None):
    """(name, device pointer, stride, component, map) of every channel of the layers whose buffer is given, in ascending byte order of name — the order of the
    file's channel list and of the pack. fb / denoised: float [H, W, 3]; aov: [H, W, 8] (crh_render_aov); *_ranked: crh_ids_resolve's [H, W, 6, 2]."""
    ch = [(n, fb, 3, i, None) for i, n in enumerate("RGB")]
    if aov is not None:
        ch += [(n, aov, 8, i, None) for i, n in enumerate(("albedo.R", "albedo.G", "albedo.B", "normal.X", "normal.Y", "normal.Z", "Z", "A"))]
    if denoised is not None:
        ch += [(f"denoised.{n}", denoised, 3, i, None) for i, n in enumerate("RGB")]
    for layer, ranked, m in ((CRYPTO_LAYERS[0], instance_ranked, instance_map), (CRYPTO_LAYERS[1], material_ranked, material_map)):
        if ranked is not None:
            ch += [(n, ranked, 2 * CRYPTO_RANKS, i, m if i % 2 == 0 else None) for i, n in enumerate(crypto_channels(layer))]
    return sorted(ch, key=lambda c: c[0].encode("utf-8"))
