"""Synthesized scenes for the tests: a shallow copy of a golden blob's crh_scene_desc in which a test replaces the node graph, the materials, the textures
and the texture coordinates, and leaves the geometry and the BVHs alone (a plain helper module, not a conftest).

    base = oracle.OracleScene(path)            # or api.Scene(path): stays untouched, it is what crh_blob_free frees
    s = SynthScene(base)
    t = s.texture(pixels)                      # uint8 / float32 [H, W, channels] in stored row order
    m = s.material(s.bsdf(DIFFUSE, s.image(t, IMAGE_NO_BILINEAR)))
    s.set_sphere_material(3, m)
    ctx.upload(s); oracle.render(s, ...); oracle.trace_rays(s, rays); oracle.camera_ray(s, x, y, 0, 1)

The object exposes .ptr and .desc like the scene classes; every array it replaces is a ctypes array it keeps alive. Graph nodes are appended, so a child's index is
below its parent's (the scene compiler demands child < parent), and a texture's data starts at a multiple of 4 bytes."""
import ctypes as C

import numpy as np

NONE = 0xFFFFFFFF
# enum crh_node_kind (include/cray_hip.h)
DIFFUSE, METAL, GLASS, PLASTIC, MIX, ADD, TRANSPARENT, EMISSION, ISOTROPIC, BACKGROUND = range(1, 11)
COLOR_CONSTANT, COLOR_IMAGE, COLOR_CHECKER, COLOR_GRADIENT, COLOR_BLACKBODY, COLOR_COMBINE, COLOR_COMBINERGB, COLOR_VECTOCOLOR = range(32, 40)
VALUE_CONSTANT, VALUE_ALPHA, VALUE_GRAYSCALE, VALUE_MATH, VALUE_FRESNEL, VALUE_RAYLENGTH = range(64, 70)
VEC_CONSTANT, VEC_NORMAL, VEC_VECMATH = 96, 97, 98
# enum mathOp (math.h:11-27) and enum vecOp (vecmath.h:11-22): field c of a math / vecMath node
(MATH_ADD, MATH_SUBTRACT, MATH_MULTIPLY, MATH_DIVIDE, MATH_POWER, MATH_LOG, MATH_SQRT, MATH_ABS, MATH_MIN, MATH_MAX, MATH_SIN, MATH_COS, MATH_TAN, MATH_TO_RADIANS,
 MATH_TO_DEGREES) = range(15)
VEC_ADD, VEC_SUBTRACT, VEC_MULTIPLY, VEC_AVERAGE, VEC_DOT, VEC_CROSS, VEC_NORMALIZE, VEC_REFLECT, VEC_LENGTH, VEC_ABS = range(10)
IMAGE_SRGB_TRANSFORM, IMAGE_NO_BILINEAR = 1, 2
BSDF_KINDS = (DIFFUSE, METAL, GLASS, PLASTIC, MIX, ADD, TRANSPARENT, EMISSION, ISOTROPIC)

# field of crh_scene_desc -> its count field
_COUNT = {"gnodes": "gnode_count", "materials": "material_count", "textures": "texture_count", "texture_data": "texture_bytes", "texcoords": "texcoord_count",
          "spheres": "sphere_count", "meshes": "mesh_count", "instances": "instance_count"}


class SynthScene:
    def __init__(self, base):
        self.base = base
        desc_type = type(base.ptr.contents)          # the ctypes mirror the loader uses (c-ray_amd/abi.py)
        self._types = {name: t._type_ for name, t in desc_type._fields_ if hasattr(t, "_type_") and hasattr(t, "contents")}
        self._desc = desc_type()
        C.memmove(C.byref(self._desc), base.ptr, C.sizeof(desc_type))
        self._ptr = C.pointer(self._desc)
        self._own = {}           # field -> the ctypes array the description points to
        self._lists = {}         # field -> records appended since the array was last rebuilt
        self._tex_bytes = None   # bytearray: texture_data with the textures added here

    # ---- the description ----
    @property
    def desc(self):
        self._flush()
        return self._desc

    @property
    def ptr(self):
        self._flush()
        return self._ptr

    def _array(self, field, extra=0):
        """The test's own copy of an array of the description, `extra` records longer than it is now."""
        count = getattr(self._desc, _COUNT[field])
        per = 2 if field == "texcoords" else 1          # texcoord_count counts xy pairs
        cur = getattr(self._desc, field)
        if field in self._own and not extra:
            return self._own[field]
        arr = (cur._type_ * max((count + extra) * per, 1))()
        if count:
            C.memmove(arr, cur, count * per * C.sizeof(cur._type_))
        self._own[field] = arr
        setattr(self._desc, field, C.cast(arr, type(cur)))
        setattr(self._desc, _COUNT[field], count + extra)
        return arr

    def _append(self, field, record):
        self._lists.setdefault(field, []).append(record)
        return getattr(self._desc, _COUNT[field]) + len(self._lists[field]) - 1

    def _flush(self):
        for field, recs in list(self._lists.items()):
            if recs:
                n = getattr(self._desc, _COUNT[field])
                arr = self._array(field, extra=len(recs))
                for k, r in enumerate(recs):
                    arr[n + k] = r
                self._lists[field] = []
        if self._tex_bytes is not None and self._own.get("texture_bytes") != len(self._tex_bytes):
            arr = (C.c_uint8 * max(len(self._tex_bytes), 1)).from_buffer_copy(bytes(self._tex_bytes) or b"\0")
            self._own["texture_bytes"] = len(self._tex_bytes)
            self._own["texture_data"] = arr
            self._desc.texture_data = C.cast(arr, C.POINTER(C.c_uint8))
            self._desc.texture_bytes = len(self._tex_bytes)

    # ---- graph nodes, children first ----
    def node(self, kind, a=NONE, b=NONE, c=NONE, f=(), children=()):
        index = self._desc.gnode_count + len(self._lists.get("gnodes", []))
        for ch in children:
            assert ch != NONE and ch < index, "children are appended before their parent"
        n = self._types["gnodes"](kind, a, b, c)
        for k, v in enumerate(f):
            n.f[k] = v
        return self._append("gnodes", n)

    def color(self, r, g, b, a=1.0):
        return self.node(COLOR_CONSTANT, f=(r, g, b, a))

    def value(self, v):
        return self.node(VALUE_CONSTANT, f=(v,))

    def image(self, tex, options=0):
        return self.node(COLOR_IMAGE, a=tex, b=options)

    def alpha(self, color):
        return self.node(VALUE_ALPHA, a=color, children=(color,))

    def grayscale(self, color):
        return self.node(VALUE_GRAYSCALE, a=color, children=(color,))

    def checker(self, a, b, scale):
        return self.node(COLOR_CHECKER, a, b, scale, children=(a, b, scale))

    def gradient(self, down, up):
        """down, up: rgba."""
        return self.node(COLOR_GRADIENT, f=tuple(down) + tuple(up))

    def blackbody(self, temperature):
        return self.node(COLOR_BLACKBODY, a=temperature, children=(temperature,))

    def combine(self, value):
        return self.node(COLOR_COMBINE, a=value, children=(value,))

    def combine_rgb(self, r, g, b):
        return self.node(COLOR_COMBINERGB, r, g, b, children=(r, g, b))

    def vec_to_color(self, vector):
        return self.node(COLOR_VECTOCOLOR, a=vector, children=(vector,))

    def math(self, op, a, b):
        """Field c is the op (enum mathOp), not a child; the unary ops ignore b, which must still be a value node."""
        return self.node(VALUE_MATH, a, b, op, children=(a, b))

    def fresnel(self, ior, normal=NONE):
        """The reference's node never reads its normal operand (fresnel.c:39-51)."""
        return self.node(VALUE_FRESNEL, a=ior, b=normal, children=[x for x in (ior, normal) if x != NONE])

    def ray_length(self):
        return self.node(VALUE_RAYLENGTH)

    def vec(self, x, y, z):
        return self.node(VEC_CONSTANT, f=(x, y, z))

    def normal(self):
        return self.node(VEC_NORMAL)

    def vecmath(self, op, a, b):
        """Field c is the op (enum vecOp), not a child; normalize, length and abs ignore b, which must still be a vector node."""
        return self.node(VEC_VECMATH, a, b, op, children=(a, b))

    def bsdf(self, kind, a=NONE, b=NONE, c=NONE):
        assert kind in BSDF_KINDS
        return self.node(kind, a, b, c, children=[x for x in (a, b, c) if x != NONE])

    def material(self, bsdf, ior=1.45, emission=(0.0, 0.0, 0.0, 0.0)):
        m = self._types["materials"]()
        for k in range(4):
            m.emission[k] = emission[k]
        m.ior, m.bsdf = ior, bsdf
        return self._append("materials", m)

    # ---- textures ----
    def drop_textures(self):
        """Forget the loaded scene's textures and their data: the textures added from here on are the scene's only ones, from index 0."""
        self._desc.texture_count = 0
        self._lists["textures"] = []
        self._tex_bytes = bytearray()

    def texture_total(self):
        """Textures of the scene, those added and not yet flushed included."""
        return self._desc.texture_count + len(self._lists.get("textures", []))

    def texture(self, pixels, has_alpha=None):
        """pixels: uint8 or float32 [H, W, channels] (channels 1, 3 or 4) in the stored row order (texture.c:39: row 0 is y = height - 1)."""
        pixels = np.ascontiguousarray(pixels)
        assert pixels.ndim == 3 and pixels.shape[2] in (1, 3, 4) and pixels.dtype in (np.uint8, np.float32)
        if self._tex_bytes is None:
            n = self._desc.texture_bytes
            self._tex_bytes = bytearray(C.string_at(self._desc.texture_data, n)) if n else bytearray()
        self._tex_bytes.extend(b"\0" * (-len(self._tex_bytes) % 4))
        t = self._types["textures"]()
        t.offset = len(self._tex_bytes)
        t.height, t.width, t.channels = pixels.shape
        t.is_float = int(pixels.dtype == np.float32)
        t.has_alpha = int(pixels.shape[2] == 4 if has_alpha is None else has_alpha)
        self._tex_bytes.extend(pixels.tobytes())
        return self._append("textures", t)

    # ---- which material an object shows ----
    def set_sphere_material(self, sphere, material):
        self._flush()
        assert material < self._desc.material_count
        self._array("spheres")[sphere].material = material

    def set_mesh_material(self, mesh, material):
        """A mesh of one material (its polygons' material index is 0) shows `material`."""
        self._flush()
        assert material < self._desc.material_count and self._desc.meshes[mesh].material_count == 1
        self._array("meshes")[mesh].material_base = material

    # ---- texture coordinates ----
    def mesh_texcoord_indices(self, mesh):
        d = self._desc
        m = d.meshes[mesh]
        idx = {d.polys[p].t[k] for p in range(m.poly_base, m.poly_base + m.poly_count) for k in range(3)}
        return np.array(sorted(i for i in idx if i >= 0), np.int64)

    def map_texcoords(self, mesh, scale, offset):
        """uv' = scale * uv + offset (float32) on the texture coordinates the mesh's polygons use, from the LOADED scene's values."""
        idx = self.mesh_texcoord_indices(mesh)
        orig = np.ctypeslib.as_array(self.base.ptr.contents.texcoords, shape=(self.base.ptr.contents.texcoord_count * 2,)).reshape(-1, 2)
        arr = self._array("texcoords")
        mine = np.ctypeslib.as_array(arr).reshape(-1, 2)
        mine[idx] = (np.float32(scale) * orig[idx] + np.float32(offset)).astype(np.float32)
        return mine[idx].copy()

    def instances(self):
        """The test's own copy of the instance records (an edited transform is the test's responsibility: the hits must still come from the oracle)."""
        return self._array("instances")

    def white_sky(self):
        """The background's colour node becomes constant white (its strength must be the constant 1)."""
        self._flush()
        g = self._array("gnodes")
        bg = g[self._desc.background]
        assert bg.kind == BACKGROUND and g[bg.b].kind == VALUE_CONSTANT and g[bg.b].f[0] == 1.0
        sky = g[bg.a]
        sky.kind = COLOR_CONSTANT
        for k in range(4):
            sky.f[k] = 1.0

