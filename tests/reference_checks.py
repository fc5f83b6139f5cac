"""Checks against what the reference itself computed, shared by several test files: the known answers of the reference's own node tests as the nodezoo_display
fixture shows them (tests/test_nodes.py, tests/test_aov.py), and the comparison of a rebuilt BVH with the reference builder's tree inside a scene blob
(tests/test_bvh_build.py, tests/test_soup_blob.py). No test lives here."""
import ctypes as C
import math

import numpy as np

ZOO_COLS, ZOO_ROWS, ZOO_PITCH = 10, 6, 0.1          # tools/gen_golden.py: write_nodezoo_scene()
W, H, FOV, CAM_Z = 320, 192, 28.0, 3.0
PI32 = float(np.float32(math.pi))
H32 = float(np.sqrt(np.float32(0.5)))

# the reference's tests/test_nodes.h —(expected r, g, b), exact unless listed in ROUGH
MATH_EXPECT = [
    (256.0, 0.0, 0.0),             # :26-40 add 128+128, -128+128; :42-56 subtract 128-128
    (-256.0, 16384.0, 1.0),        # subtract -128-128; :58-66 multiply; :68-82 divide 128/128
    (-128.0, 65536.0, -128.0),     # divide -128/1; :84-103 power 2^16, (-128)^1
    (1.0, 0.0, 1.0),               # power 128^0; :105-129 log10 1, 10
    (2.0, 3.0, 4.0),               # log10 100, 1000, 10000
    (3.0, 128.0, 128.0),           # :131-139 sqrt 9; :141-153 abs
    (-128.0, 42.0, 128.0),         # :155-169 min; :171-185 max -128,128
    (128.0, 0.0, -1.0),            # max 128,42; :188-196 sin(pi) ~ 0; :198-206 cos(pi) ~ -1
    (0.0, PI32, 180.0),            # :208-216 tan(pi) ~ 0; :218-226 toRadians(180) ~ pi; :228-236 toDegrees(pi) ~ 180
]
VEC_EXPECT = [
    (2.0, 4.0, 6.0), (0.0, 0.0, 0.0), (1.0, 4.0, 9.0), (2.5, 2.5, 2.5),     # :245-303 add, subtract, multiply, average
    (0.0, 0.0, 0.0),                                                         # :305-326 dot: the float result is not the vector
    (0.0, 0.0, 1.0),                                                         # :328-341 cross
    tuple(float(v) for v in (np.float32([1, 2, 3]) / np.sqrt(np.float32(14.0)))),   # :343-353 normalize
    (H32, -H32, 0.0),                                                        # :355-371 reflect
    (0.0, 0.0, 0.0),                                                         # :373-383 length
    (10.0, 2.0, 3.0),                                                        # :385-395 abs
]
EXPECT = {i: v for i, v in enumerate(MATH_EXPECT)}
EXPECT.update({9 + i: v for i, v in enumerate(MATH_EXPECT)})
EXPECT.update({18 + i: v for i, v in enumerate(VEC_EXPECT)})
EXPECT.update({28 + i: v for i, v in enumerate(VEC_EXPECT)})
LIBM = {2, 3, 4, 7, 8}            # math spheres whose values go through powf / log10f / sinf / cosf / tanf (roughly_equals in the reference's tests too)


def sphere_pixel(i):
    """Image (row, col) of the centre of nodezoo sphere i (stored rows run top-down: texture.c:24-28)."""
    col, row = i % ZOO_COLS, i // ZOO_COLS
    x, y = (col - (ZOO_COLS - 1) / 2) * ZOO_PITCH, ((ZOO_ROWS - 1) / 2 - row) * ZOO_PITCH
    pix = 2.0 * math.tan(math.radians(FOV) / 2.0) / W * CAM_Z
    return int(round(H / 2 - y / pix - 0.5)), int(round(x / pix + W / 2 - 0.5))


def sphere_value(img, i):
    """Colour shown by sphere i: per-channel median of the 5 x 5 pixels around its centre (a bounce that hits a neighbour is black)."""
    r, c = sphere_pixel(i)
    return np.median(img[r - 2:r + 3, c - 2:c + 3].reshape(-1, 3), axis=0)


def check_known_answers(img):
    """Exact for everything IEEE arithmetic decides; the reference's own `roughly_equals` for the values that pass through libm."""
    for i, want in EXPECT.items():
        got = sphere_value(img, i)
        if i < 18 and (i % 9) in LIBM:
            assert np.allclose(got, want, rtol=1e-6, atol=2e-7), (i, got, want)
        else:
            assert np.array_equal(got, np.float32(want)), (i, got, want)


def mesh_views(desc, m):
    """(reference nodes uint32[n, 8], reference prim order int32[count], polys pointer, count) of mesh m."""
    mesh = desc.meshes[m]
    nodes = np.ctypeslib.as_array(C.cast(desc.nodes, C.POINTER(C.c_uint32)), shape=(int(desc.node_count), 8))
    prims = np.ctypeslib.as_array(C.cast(desc.prim_indices, C.POINTER(C.c_int32)), shape=(int(desc.prim_index_count),))
    polys = C.cast(desc.polys, C.c_void_p).value + 40 * mesh.poly_base
    n, count = mesh.node_count, mesh.poly_count
    return nodes[mesh.node_base:mesh.node_base + n], prims[mesh.prim_base:mesh.prim_base + (count if n else 0)], polys, count


def assert_same_bvh(nodes, prims, ref_nodes, ref_prims, what):
    assert nodes.shape == ref_nodes.shape, (what, nodes.shape, ref_nodes.shape)
    leaf = ((ref_nodes[:, 7] >> 30) & 1) == 1
    assert np.array_equal(((nodes[:, 7] >> 30) & 1) == 1, leaf), what
    assert np.array_equal(nodes[:, :7], ref_nodes[:, :7]), what           # bounds (bit patterns) + first child / first prim
    assert np.array_equal(nodes[leaf, 7] & 0x7FFFFFFF, ref_nodes[leaf, 7] & 0x7FFFFFFF), what
    assert np.array_equal(prims, ref_prims), what
