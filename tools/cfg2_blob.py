#!/usr/bin/env python3
"""cfg2_blob.py — the scene of BASELINE.json configs[1] (input/hdr.json, bench.py's headline workload) as a blob, rebuilt WITHOUT the reference tree.
BENCH / TEST INFRASTRUCTURE.

The 70 MB blob crh-flatten writes is mostly the generated 524 288-triangle stand-in statue (tools/gen_assets.py), its BVH and the reference's HDR
environment map (1024 x 512 float RGB: photographic data, 1.2 MB even losslessly packed — too large for a fixture). The rest — camera, materials, node
graph, instances, the grid texture — is a 15 kB data fixture, tests/golden/cfg2_hdr.skel.xz: that blob with the statue's sections and the map's texels
zeroed. fill() writes them again:
  vertices / normals  gen_assets.write_statue's OBJ text, read back as the reference's OBJ loader reads it (atof, then float);
  polys               its faces (`f v//n`): vertex index + VERTEX_BASE, normal index as is, texcoords = the mesh's TEXCOORD, the skeleton's poly bits;
  BVH                 the restated reference builder (oracle/bvh_oracle.c) over those triangles; nodes and prim order as the flattener stores them;
  environment map     the texels given (the reference's: the result is the flattened blob byte for byte — tests/test_bench_line.py) or, by
                      default, standin_sky(): a generated sky of the same size. The map is read only by rays that leave the scene, which ends
                      their paths (pathtrace.c: roulette on the surface's attenuation), so the stand-in gives the same paths and the same rays;
                      only the radiance they carry differs.
rebuild() writes the stand-in form and refuses to write anything whose md5 is not the one recorded in the skeleton.

    python tools/cfg2_blob.py out.blob                    rebuild (stand-in environment map)
    python tools/cfg2_blob.py --skeleton cfg2_hdr.blob    write tests/golden/cfg2_hdr.skel.xz from a flattened blob (needs the reference)
"""
import hashlib
import json
import lzma
import os
import struct
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKELETON = os.path.join(REPO, "tests", "golden", "cfg2_hdr.skel.xz")
HEADER_BYTES = 180                          # sizeof(struct blob_header), c-ray_amd/host/scene_blob.c
SEC_NODES, SEC_PRIMS, SEC_POLYS, SEC_VERTS, SEC_NORMALS = 0, 1, 2, 3, 4
SEC_COUNT = 13
MESH = 1                                    # the statue: mesh 1 of hdr.json (mesh 0 is the floor quad)
VERTEX_BASE = 8                             # OBJ vertex i (1-based) is vertices[i + 8]: the floor's 4 vertices and 5 of slack come first
TEXCOORD = 3                                # a mesh without texcoords points at the last texcoord of the floor (the flattener's default)
STATUE_VERTICES = 512 * 512 + 2             # gen_assets.write_statue(rows=512, cols=512): the rings and the two poles (as many normals)


def sections(buf):
    """[(elem_size, count, offset)] of the section table of a blob image."""
    out = []
    for i in range(SEC_COUNT):
        sid, es, n, off = struct.unpack_from("<IIQQ", buf, HEADER_BYTES + 24 * i)
        assert sid == i, "not a scene blob of this ABI"
        out.append((es, n, off))
    return out


def view(buf, sec, dtype, width):
    es, n, off = sec
    return np.frombuffer(buf, dtype, count=n * width, offset=off).reshape(n, width)


def statue_ranges(buf):
    """Row ranges of the statue in the nodes, prims / polys, vertices and normals sections (from its mesh record)."""
    secs = sections(buf)
    mesh = view(buf, secs[7], np.uint32, 12)[MESH]            # crh_mesh: node_base, node_count, prim_base, poly_base, poly_count, ...
    node_base, node_count, prim_base, poly_base, poly_count = (int(x) for x in mesh[:5])
    assert prim_base == poly_base
    return secs, (node_base, node_count), (poly_base, poly_count)


def read_statue_obj(path):
    """(vertices float32 [n, 3], normals float32 [n, 3], faces int32 [m, 3] of 1-based `f v//n` indices with v == n) as the OBJ loader reads them."""
    vs, ns, fs = [], [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                vs.append(line.split()[1:4])
            elif line.startswith("vn "):
                ns.append(line.split()[1:4])
            elif line.startswith("f "):
                fs.append([c.split("//")[0] for c in line.split()[1:4]])
    to32 = lambda rows: np.array(rows, dtype=np.float64).astype(np.float32)          # atof (double) -> float, as the loader does
    return to32(vs), to32(ns), np.array(fs, dtype=np.int32)


def env_map_range(buf):
    """(byte offset, width, height) of the float RGB environment map's texels in a blob image."""
    secs = sections(buf)
    tex = view(buf, secs[11], np.uint32, 8)                 # crh_texture: offset (u64), width, height, channels, is_float, has_alpha, pad
    (i,) = [k for k in range(len(tex)) if tex[k, 5] == 1 and tex[k, 4] == 3]
    return secs[12][2] + int(tex[i, 0]) + (int(tex[i, 1]) << 32), int(tex[i, 2]), int(tex[i, 3])


def standin_sky(width, height):
    """float32 [height, width, 3]: a blue-to-white sky with a warm sun, from + - * / only (exactly rounded in float32: the same bits on every CPU)."""
    f = np.float32
    v = ((np.arange(height, dtype=f) + f(0.5)) / f(height))[:, None]
    u = ((np.arange(width, dtype=f) + f(0.5)) / f(width))[None, :]
    d = (u - f(0.3)) * (u - f(0.3)) * f(4.0) + (v - f(0.3)) * (v - f(0.3)) * f(16.0)
    sun = f(12.0) / (f(1.0) + f(400.0) * d)
    sky = np.empty((height, width, 3), f)
    sky[:, :, 0] = f(0.35) + f(0.65) * v + sun
    sky[:, :, 1] = f(0.55) + f(0.45) * v + f(0.8) * sun
    sky[:, :, 2] = f(1.0) + f(0.1) * v + f(0.5) * sun
    return sky


def load_skeleton():
    with lzma.open(SKELETON) as f:
        meta_len, = struct.unpack("<I", f.read(4))
        meta = json.loads(f.read(meta_len))
        return meta, bytearray(f.read())


def fill(buf, meta, env=None):
    """Write the statue, its BVH and the environment map (`env`, float32 [h, w, 3]; None = standin_sky) into a skeleton image, in place."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import gen_assets
    import oracle_py
    secs, (node_base, node_count), (poly_base, poly_count) = statue_ranges(buf)
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "venusscaled.obj")
        gen_assets.write_statue(obj)
        verts, norms, faces = read_statue_obj(obj)
    assert len(faces) == poly_count and len(verts) == len(norms) == STATUE_VERTICES
    V = view(buf, secs[SEC_VERTS], np.float32, 3)
    V.flags.writeable = True
    V[VERTEX_BASE + 1:VERTEX_BASE + 1 + len(verts)] = verts
    Nrm = view(buf, secs[SEC_NORMALS], np.float32, 3)
    Nrm.flags.writeable = True
    Nrm[1:1 + len(norms)] = norms
    P = view(buf, secs[SEC_POLYS], np.int32, 10)
    P.flags.writeable = True
    polys = P[poly_base:poly_base + poly_count]
    polys[:, 0:3] = faces + VERTEX_BASE
    polys[:, 3:6] = faces
    polys[:, 6:9] = TEXCOORD
    polys[:, 9] = meta["poly_bits"]
    polys = np.ascontiguousarray(polys)
    nodes, prims = oracle_py.bvh_build_triangles(polys.ctypes.data, np.ascontiguousarray(V).ctypes.data, poly_count)
    assert len(nodes) == node_count, (len(nodes), node_count)
    Nd = view(buf, secs[SEC_NODES], np.uint32, 8)
    Nd.flags.writeable = True
    Nd[node_base:node_base + node_count] = nodes
    Pr = view(buf, secs[SEC_PRIMS], np.int32, 1)
    Pr.flags.writeable = True
    Pr[poly_base:poly_base + poly_count, 0] = prims
    off, w, h = env_map_range(buf)
    texels = np.ascontiguousarray(standin_sky(w, h) if env is None else env, dtype=np.float32)
    assert texels.shape == (h, w, 3)
    buf[off:off + texels.nbytes] = texels.tobytes()
    return buf


def rebuild(out_path):
    meta, buf = load_skeleton()
    fill(buf, meta)
    digest = hashlib.md5(buf).hexdigest()
    if digest != meta["md5_standin"]:
        raise RuntimeError(f"cfg2_blob: rebuilt blob has md5 {digest}, the recorded one {meta['md5_standin']}: not written")
    tmp_out = out_path + ".tmp"
    with open(tmp_out, "wb") as f:
        f.write(buf)
    os.replace(tmp_out, out_path)
    return out_path


def make_skeleton(blob_path, out=SKELETON):
    buf = bytearray(open(blob_path, "rb").read())
    secs, (node_base, node_count), (poly_base, poly_count) = statue_ranges(buf)
    meta = {"md5_flattened": hashlib.md5(buf).hexdigest(), "poly_bits": int(view(buf, secs[SEC_POLYS], np.uint32, 10)[poly_base, 9])}
    off, w, h = env_map_range(buf)

    def zero(sec, first, rows):
        es, _n, off = secs[sec]
        buf[off + first * es:off + (first + rows) * es] = bytes(rows * es)
    zero(SEC_NODES, node_base, node_count)
    zero(SEC_PRIMS, poly_base, poly_count)
    zero(SEC_POLYS, poly_base, poly_count)
    zero(SEC_VERTS, VERTEX_BASE + 1, STATUE_VERTICES)
    zero(SEC_NORMALS, 1, STATUE_VERTICES)
    buf[off:off + w * h * 12] = bytes(w * h * 12)
    meta["md5_standin"] = hashlib.md5(fill(bytearray(buf), meta)).hexdigest()
    head = json.dumps(meta).encode()
    with lzma.open(out, "wb", preset=9 | lzma.PRESET_EXTREME) as f:
        f.write(struct.pack("<I", len(head)) + head + bytes(buf))
    return out


if __name__ == "__main__":
    if sys.argv[1] == "--skeleton":
        print(make_skeleton(sys.argv[2]))
    else:
        print(rebuild(sys.argv[1]))
