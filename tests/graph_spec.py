"""What the tests on synthesized node graphs share (tests/test_graph_edges.py, tests/test_node_edges.py, tests/test_bsdf_edges.py; no test lives here).

The restatement: the albedo rule (include/cray_hip.h), the reference's texture fetch (texture.c:32-79, image.c:31-48, alpha.c, grayscale.c, color.h) and its
node kinds in NumPy float32 — recursive, no stack limit, (size_t) wraps as Python integers modulo 2^64, powf and the other libm functions from the C library. Its
input is the oracle's hit record of each pixel's camera ray. The bit-exact tests depend on the order of the float32 operations in it.

Around it: the views of nodezoo_display the scenes are synthesized in (tests/scene_synth.py) and their camera rays, the edge values and leaves the edge tests
build their graphs from, and the device side — a description handed to the product library, its albedo buffer, the comparison with the restatement."""
import ctypes as C

import numpy as np
import pytest

from conftest import resize_camera
from firsthit_spec import geometry_expected
from scene_synth import (ADD, DIFFUSE, EMISSION, GLASS, IMAGE_NO_BILINEAR, IMAGE_SRGB_TRANSFORM, ISOTROPIC, METAL, MIX, NONE, PLASTIC, TRANSPARENT, COLOR_BLACKBODY,
                         COLOR_CHECKER, COLOR_COMBINE, COLOR_COMBINERGB, COLOR_CONSTANT, COLOR_GRADIENT, COLOR_IMAGE, COLOR_VECTOCOLOR, VALUE_ALPHA, VALUE_CONSTANT,
                         VALUE_FRESNEL, VALUE_GRAYSCALE, VALUE_MATH, VALUE_RAYLENGTH, VEC_ADD, VEC_CONSTANT, VEC_MULTIPLY, VEC_NORMAL, VEC_VECMATH, SynthScene)

F = np.float32
S, NB = IMAGE_SRGB_TRANSFORM, IMAGE_NO_BILINEAR

# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------------
_libm = C.CDLL("libm.so.6")
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]


for _f in ("log10f", "logf", "sinf", "cosf", "tanf"):
    getattr(_libm, _f).restype = C.c_float
    getattr(_libm, _f).argtypes = [C.c_float]


def powf(x, y):
    """The C library's powf on every element (numpy's power is not that function), y a scalar or an array like x; one call per distinct pair of bit patterns."""
    x = np.ascontiguousarray(x, F)
    y = np.ascontiguousarray(np.broadcast_to(F(y), x.shape))
    key = (x.view(np.uint32).astype(np.uint64) << np.uint64(32)) | y.view(np.uint32).astype(np.uint64)
    pairs, inverse = np.unique(key, return_inverse=True)
    xs, ys = (pairs >> np.uint64(32)).astype(np.uint32).view(F), (pairs & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(F)
    vals = np.array([_libm.powf(float(a), float(b)) for a, b in zip(xs, ys)], F)
    return vals[inverse.reshape(-1)].reshape(x.shape)


def libm1(name, x):
    """A one-argument function of the C library on every element of a float32 array; one call per distinct bit pattern."""
    x = np.ascontiguousarray(x, F)
    fn = getattr(_libm, name)
    bits, inverse = np.unique(x.view(np.uint32), return_inverse=True)
    vals = np.array([fn(float(v)) for v in bits.view(F)], F)
    return vals[inverse.reshape(-1)].reshape(x.shape)


PI = F(3.141592653589793238462643383279502)          # includes.h:13, a float


def rmin(a, b):
    """includes.h:20: ((a) < (b)) ? (a) : (b) — b when either is NaN, b for (+0, -0) and (-0, +0)."""
    return np.where(a < b, a, b)


def rmax(a, b):
    """includes.h:21: ((a) > (b)) ? (a) : (b)."""
    return np.where(a > b, a, b)


def vdot(a, b):
    """vector.h:92-94: v1.x * v2.x + v1.y * v2.y + v1.z * v2.z, every operation rounded to float32, left to right."""
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def vlength(a):
    return np.sqrt(vdot(a, a))          # vector.h:152-164


def vnormalize(a):
    return a / vlength(a)[:, None]          # vector.h:173-176: three divisions by the length


def vcross(a, b):
    """vector.h:122-127."""
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def vreflect(i, n):
    """vector.h:211-213: vecSub(I, vecScale(N, vecDot(N, I) * 2.0f))."""
    return i - n * (vdot(n, i) * F(2.0))[:, None]


def color_for_kelvin(kelvin):
    """color.c:28-70 on a float32 array: [n, 4]. Every comparison is the source's own, so a NaN takes the branch the source's comparison gives it and
    passes through both clamps (x < 0 and x > 255 are false for it)."""
    with np.errstate(all="ignore"):
        temp = np.where(kelvin >= F(40000.0), F(40000.0), kelvin) / F(100.0)

        def clamp(x):
            x = np.where(x < F(0.0), F(0.0), x)
            return np.where(x > F(255.0), F(255.0), x)
        low = temp <= F(66.0)
        r = np.where(low, F(255.0), clamp(F(329.698727446) * powf(temp - F(60.0), -0.1332047592)))
        g = clamp(np.where(low, F(99.4708025861) * libm1("logf", temp) - F(161.1195681661), F(288.1221695283) * powf(temp - F(60.0), -0.0755148492)))
        b = np.where(temp >= F(66.0), F(255.0), np.where(temp <= F(19.0), F(0.0), clamp(F(138.5177312231) * libm1("logf", temp - F(10.0)) - F(305.0447927307))))
        return np.stack([r / F(255.0), g / F(255.0), b / F(255.0), np.zeros_like(r)], axis=1).astype(F)


def schlick(cosine, ior):
    """vector.h:268-272."""
    r0 = (F(1.0) - ior) / (F(1.0) + ior)
    r0 = r0 * r0
    return r0 + (F(1.0) - r0) * powf(F(1.0) - cosine, 5.0)


def srgb_to_linear(c):
    """color.h:68-74 (a negative channel — a filtered fetch with a negative blend factor gives some — takes the linear branch)."""
    low = c <= F(0.04045)
    out = c / F(12.92)
    if (~low).any():
        out[~low] = powf((c[~low] + F(0.055)) / F(1.055), 2.4)
    return out


def cmix(a, b, t):
    """color.h:53-55: colorAdd(colorCoef(1 - t, a), colorCoef(t, b)), every operation in float32."""
    t = np.asarray(t, F)[..., None]
    return (F(1.0) - t) * a + t * b


def size_t(i):
    return int(i) % (1 << 64)


class Restatement:
    """albedo(material root, hits) on the node graph of a scene description. `probes` collects what every image fetch saw (test f's conditions)."""

    def __init__(self, desc):
        self.d = desc
        self._tex = {}
        self.probes = []

    def texels(self, t):
        """float32 [height, width, 4]: [y, x] is textureGetPixelInternal(x, y) (texture.c:32-63)."""
        if t not in self._tex:
            T = self.d.textures[t]
            w, h, ch = T.width, T.height, T.channels
            addr = C.addressof(self.d.texture_data.contents) + T.offset
            if T.is_float:
                a = np.frombuffer(C.string_at(addr, w * h * ch * 4), F)
            else:
                a = np.frombuffer(C.string_at(addr, w * h * ch), np.uint8).astype(F) / F(255.0)
            a = a.reshape(h, w, ch)[::-1]          # the stored row of y is height - 1 - y
            out = np.ones((h, w, 4), F)
            out[..., 0:3] = a[..., 0:3] if ch > 1 else a
            if ch == 4 and T.has_alpha:
                out[..., 3] = a[..., 3]
            self._tex[t] = out
        return self._tex[t]

    def image(self, n, uv):
        """image.c:31-48 on uv [n, 2]."""
        if n.a == NONE:
            return np.tile(F([1.0, 0.0, 0.5, 1.0]), (len(uv), 1))          # warningMaterial().diffuse (material.c:38)
        T = self.d.textures[n.a]
        W, H = int(T.width), int(T.height)
        tex = self.texels(n.a)
        probe = {"tex": int(n.a), "options": int(n.b), "width": W, "height": H}
        if n.b & IMAGE_NO_BILINEAR:
            x, y = uv[:, 0] * F(W), uv[:, 1] * F(H)
            assert (x >= 0).all() and (y >= 0).all(), "a nearest fetch at a negative uv is out of scope ((size_t) of a negative float)"
            xi = np.array([size_t(v) % W for v in x], np.int64)          # textureGetPixel(.., false): (size_t)x, then x % width
            yi = np.array([size_t(v) % H for v in y], np.int64)
            out = tex[yi, xi].copy()
            probe.update(x=x, y=y, tx=xi, ty=yi)
        else:
            x, y = uv[:, 0] * F(W), uv[:, 1] * F(H)
            xc, yc = x - F(0.5), y - F(0.5)
            assert (np.abs(xc) < 2.0 ** 31).all() and (np.abs(yc) < 2.0 ** 31).all(), "a filtered fetch with |uv * size| >= 2^31 is out of scope ((int) of it)"
            xint, yint = np.trunc(xc).astype(np.int64), np.trunc(yc).astype(np.int64)          # (int): towards zero
            x0 = np.array([size_t(i) % W for i in xint], np.int64)
            x1 = np.array([size_t(i + 1) % W for i in xint], np.int64)
            y0 = np.array([size_t(i) % H for i in yint], np.int64)
            y1 = np.array([size_t(i + 1) % H for i in yint], np.int64)
            fx, fy = xc - xint.astype(F), yc - yint.astype(F)
            out = cmix(cmix(tex[y0, x0], tex[y0, x1], fx), cmix(tex[y1, x0], tex[y1, x1], fx), fy)
            probe.update(xint=xint, yint=yint, fx=fx, fy=fy, tx=x0, ty=y0, tx1=x1, ty1=y1)
        if n.b & IMAGE_SRGB_TRANSFORM:
            probe["fetched"] = out[:, 0:3].copy()
            out[:, 0:3] = srgb_to_linear(out[:, 0:3])
        self.probes.append(probe)
        return out

    def color(self, j, hits):
        n = self.d.gnodes[j]
        if n.kind == COLOR_CONSTANT:
            return np.tile(F(list(n.f[0:4])), (len(hits), 1))
        if n.kind == COLOR_IMAGE:
            return self.image(n, hits["uv"])
        with np.errstate(all="ignore"):
            if n.kind == COLOR_CHECKER:          # checker.c:31-54: one branch on sines < 0 (a NaN picks B); the point form where uv.x < 0
                coef = self.value(n.c, hits)
                uv, p = hits["uv"], hits["point"]
                mapped = libm1("sinf", coef * uv[:, 0]) * libm1("sinf", coef * uv[:, 1])
                unmapped = libm1("sinf", coef * p[:, 0]) * libm1("sinf", coef * p[:, 1]) * libm1("sinf", coef * p[:, 2])
                sines = np.where(uv[:, 0] >= 0, mapped, unmapped)
                return np.where((sines < F(0.0))[:, None], self.color(n.a, hits), self.color(n.b, hits))
            if n.kind == COLOR_GRADIENT:          # gradient.c:40-45
                t = F(0.5) * (vnormalize(hits["dir"])[:, 1] + F(1.0))
                return (F(1.0) - t)[:, None] * F(list(n.f[0:4])) + t[:, None] * F(list(n.f[4:8]))
            if n.kind == COLOR_BLACKBODY:          # blackbody.c:38-42
                return color_for_kelvin(self.value(n.a, hits))
            if n.kind == COLOR_COMBINE:          # combine.c:38-43
                v = self.value(n.a, hits)
                return np.stack([v, v, v, np.ones_like(v)], axis=1)
            if n.kind == COLOR_COMBINERGB:          # combinergb.c:42-51
                r = self.value(n.a, hits)
                return np.stack([r, self.value(n.b, hits), self.value(n.c, hits), np.ones_like(r)], axis=1)
            if n.kind == COLOR_VECTOCOLOR:          # vectocolor.c:38-43
                v = self.vector(n.a, hits)
                return np.concatenate([v, np.zeros((len(v), 1), F)], axis=1)
        raise NotImplementedError(f"colour node kind {n.kind}")

    def vector(self, j, hits):
        """float32 [n, 3]: the .v of the node's vectorValue (dot and length answer in .f, their .v is zero: vecmath.c:60-62, 72-74)."""
        n = self.d.gnodes[j]
        if n.kind == VEC_CONSTANT:
            return np.tile(F(list(n.f[0:3])), (len(hits), 1))
        if n.kind == VEC_NORMAL:
            return hits["normal"].astype(F)
        if n.kind == VEC_VECMATH:          # vecmath.c:41-81
            a, b = self.vector(n.a, hits), self.vector(n.b, hits)
            with np.errstate(all="ignore"):
                if n.c == 0:
                    return a + b
                if n.c == 1:
                    return a - b
                if n.c == 2:
                    return a * b
                if n.c == 3:
                    return (a + b) * F(0.5)
                if n.c in (4, 8):
                    return np.zeros_like(a)
                if n.c == 5:
                    return vcross(a, b)
                if n.c == 6:
                    return vnormalize(a)
                if n.c == 7:
                    return vreflect(a, b)
                if n.c == 9:
                    return np.abs(a)
        raise NotImplementedError(f"vector node kind {n.kind} op {n.c}")

    @staticmethod
    def math(op, a, b):
        """math.c:42-95."""
        with np.errstate(all="ignore"):
            if op == 0:
                return a + b
            if op == 1:
                return a - b
            if op == 2:
                return a * b
            if op == 3:
                return a / b
            if op == 4:
                return powf(a, b)
            if op == 5:
                return libm1("log10f", a)
            if op == 6:
                return np.sqrt(a)
            if op == 7:
                return np.abs(a)
            if op == 8:
                return rmin(a, b)
            if op == 9:
                return rmax(a, b)
            if op in (10, 11, 12):
                return libm1(("sinf", "cosf", "tanf")[op - 10], a)
            if op == 13:
                return (a * PI) / F(180.0)          # transforms.c:18-20
            if op == 14:
                return a * (F(180.0) / PI)          # transforms.c:22-24
        raise NotImplementedError(f"math op {op}")

    def value(self, j, hits):
        n = self.d.gnodes[j]
        if n.kind == VALUE_CONSTANT:
            return np.full(len(hits), n.f[0], F)
        if n.kind == VALUE_ALPHA:
            return self.color(n.a, hits)[:, 3].copy()
        if n.kind == VALUE_GRAYSCALE:
            # color.h:42-45: 0.587 and 0.114 are double constants, so the sum is carried in double; sqrtf takes it as a float. The source's powf(x, 2) is x * x
            # in the reference binary (its compiler folds the constant exponent; the C library's powf(x, 2) differs from x * x by an ulp for one x in 1300)
            c = self.color(n.a, hits)
            with np.errstate(all="ignore"):
                s = (F(0.299) * (c[:, 0] * c[:, 0])).astype(np.float64) + 0.587 * (c[:, 1] * c[:, 1]).astype(np.float64) + 0.114 * (c[:, 2] * c[:, 2]).astype(np.float64)
                return np.sqrt(s.astype(F))
        if n.kind == VALUE_MATH:
            return self.math(n.c, self.value(n.a, hits), self.value(n.b, hits)).astype(F)
        if n.kind == VALUE_RAYLENGTH:          # raylength.c:36-40
            return hits["distance"].astype(F)
        if n.kind == VALUE_FRESNEL:          # fresnel.c:39-51 (the normal operand is never read)
            with np.errstate(all="ignore"):
                ior = self.value(n.a, hits)
                d, nrm = hits["dir"], hits["normal"]
                dot, length = vdot(d, nrm), vlength(d)
                cosine = np.where(dot > F(0.0), ior * dot / length, -(dot / length))
                return schlick(cosine, ior)
        raise NotImplementedError(f"value node kind {n.kind}")

    def albedo(self, j, hits):
        """float32 [n, 3]: the rule of include/cray_hip.h (crh_render_aov), recursively."""
        n = self.d.gnodes[j]
        if n.kind in (DIFFUSE, METAL, GLASS, TRANSPARENT, ISOTROPIC):
            return self.color(n.a, hits)[:, 0:3].copy()
        if n.kind == EMISSION:
            return self.color(n.a, hits)[:, 0:3] * self.value(n.b, hits)[:, None]
        if n.kind == PLASTIC:
            return self.albedo(n.c, hits)
        if n.kind == MIX:
            return cmix(self.albedo(n.a, hits), self.albedo(n.b, hits), self.value(n.c, hits))
        if n.kind == ADD:
            return self.albedo(n.a, hits) + self.albedo(n.b, hits)
        raise NotImplementedError(f"bsdf node kind {n.kind}")

    def frame(self, hits):
        """Albedo of every pixel of a hit array [h, w] (a miss: zeros), material by material."""
        out = np.zeros(hits.shape + (3,), F)
        hit = hits["inst"] >= 0
        for m in np.unique(hits["material"][hit]):
            sel = hit & (hits["material"] == m)
            out[sel] = self.albedo(self.d.materials[int(m)].bsdf, hits[sel])
        return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The views of nodezoo_display and their camera rays
# ---------------------------------------------------------------------------------------------------------------------------------------------------
PLANE, CUBE = 1, 0          # nodezoo's meshes: the textured plane, the cube without texture coordinates
SPHERES_W, SPHERES_H = 160, 96
MESH_W, MESH_H = 120, 72
# the plane seen from behind (the spheres stand in front of it), far enough to show all of it
MESH_CAMERA_A = (-1.0, 0.0, 0.0, 0.62, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 8.3)


def size_of(view):
    return {"mesh": (MESH_W, MESH_H), "spheres": (SPHERES_W, SPHERES_H), "texwrap": (160, 100)}[view]


_rays = {}


def scene_hits(oracle, s, view, passes=(0,), max_passes=1, dirs=False):
    """hits[k][row, col] of the camera rays of `passes` (the rays depend on the view alone and are shared by the variants). With `dirs`, every record also
    carries its ray's direction as the field "dir" (incident.direction of the hit record: fresnel.c and gradient.c read it)."""
    w, h = size_of(view)
    out = []
    for p in passes:
        key = (view, p, max_passes)
        if key not in _rays:
            _rays[key] = np.array([[oracle.camera_ray(s, x, y, p, max_passes) for x in range(w)] for y in reversed(range(h))], F)
        hits = oracle.trace_rays(s, _rays[key].reshape(-1, 6)).reshape(h, w)
        if dirs:
            wide = np.zeros(hits.shape, hits.dtype.descr + [("dir", "<f4", (3,))])
            for name in hits.dtype.names:
                wide[name] = hits[name]
            wide["dir"] = _rays[key][..., 3:6]
            hits = wide
        out.append(hits)
    return np.stack(out)


@pytest.fixture(scope="module")
def base(oracle, golden_blob):
    b = oracle.OracleScene(golden_blob("nodezoo_display"))
    yield b
    b.close()


def white_sky_selection(oracle, s, hits, view):
    """The oracle's render of the description under a constant white sky, 1 sample, 2 bounces: where the first hit is a diffuse root and the second ray escaped
    (the pixel is not black), the pixel IS the albedo."""
    w, h = size_of(view)
    s.white_sky()
    img = oracle.render(s, w, h, 1, 2, threads=1)[0]
    d = s.desc
    diffuse = np.array([d.gnodes[d.materials[m].bsdf].kind == DIFFUSE for m in range(d.material_count)])
    hit = hits["inst"] >= 0
    sel = hit & diffuse[np.where(hit, hits["material"], 0)] & (img != 0).any(axis=2)
    return img, sel


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Edge values and the leaves that carry them into a graph
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def f32(x):
    return float(F(x))


FLT_MAX, FLT_MIN = f32(np.finfo(F).max), f32(np.finfo(F).tiny)
SUB_MIN = f32(np.finfo(F).smallest_subnormal)          # 1.4e-45
SUB_MAX = f32(np.nextafter(F(FLT_MIN), F(0)))          # the largest subnormal
INF, NAN = float("inf"), float("nan")


def bits(x):
    return int(F(x).view(np.uint32))


class Leaves:
    """dynamic: a value is alpha(image(1 x 1 float RGBA texture, NO_BILINEAR)), a vector is add(C, multiply(normal, 0)); otherwise constants."""

    def __init__(self, s, dynamic, textures=None):
        self.s, self.dynamic, self.textures = s, dynamic, textures          # textures: the scene's shared image textures (new_scene), for the checkers' colours
        self._tex = {}

    def val(self, x):
        s = self.s
        if not self.dynamic:
            return s.value(x)
        if bits(x) not in self._tex:
            self._tex[bits(x)] = s.texture(np.array([[[0.25, 0.5, 0.75, x]]], F))
        return s.alpha(s.image(self._tex[bits(x)], NB))

    def vec(self, x, y, z):
        s = self.s
        assert not any(bits(v) == bits(-0.0) for v in (x, y, z))
        if not self.dynamic:
            return s.vec(x, y, z)
        return s.vecmath(VEC_ADD, s.vec(x, y, z), s.vecmath(VEC_MULTIPLY, s.normal(), s.vec(0.0, 0.0, 0.0)))


def shared_textures(s):
    """Two image textures for the checkers' colours, and as many more as the fixture's own (unshown) image nodes need to stay valid."""
    rng = np.random.default_rng(20261018)
    a = rng.integers(0, 256, (6, 7, 4), dtype=np.uint8)
    tex = {"rgba7x6": s.texture(a), "rgbaf2x2": s.texture(rng.random((2, 2, 4), dtype=F))}
    while s.texture_total() < s.base.desc.texture_count:
        s.texture(np.zeros((1, 1, 3), np.uint8))
    return tex


def new_scene(base, view):
    s = SynthScene(base)
    s.drop_textures()
    tex = shared_textures(s)
    cam = s.desc.camera
    if view == "spheres":
        resize_camera(s, *size_of("spheres"))
    else:
        for k in range(12):
            cam.A[k] = MESH_CAMERA_A[k]
        resize_camera(s, *size_of(view))
    return s, tex


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The device side
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class ForLibrary:
    """The description as the product library's ctypes mirror types it (the oracle binding may hold a mirror module of its own)."""

    def __init__(self, pkg, s):
        self.scene = s
        self.ptr = C.cast(s.ptr, C.POINTER(pkg.abi.SceneDesc))


def gpu_aov(pkg, ctx, s, w, h, samples):
    ctx.upload(ForLibrary(pkg, s))
    buf = ctx.aov_buffer(w, h)
    try:
        ctx.render_aov(buf, w, h, samples)
        return ctx.download_aov(buf, w, h)
    finally:
        ctx.L.crh_aov_free(ctx.h, buf)
        ctx._owned_aovs.remove(buf)


def same_bits(a, b, nan_equal=False):
    """Elementwise: the same bits — with `nan_equal`, also a NaN against a NaN of any payload or sign (x86 and the GPU produce different default NaNs;
    tests/test_exact_math.py sets the same bar)."""
    same = np.ascontiguousarray(a, F).view(np.uint32) == np.ascontiguousarray(b, F).view(np.uint32)
    return same | (np.isnan(a) & np.isnan(b)) if nan_equal else same


def assert_aov(got, want_albedo, hits, passes, what, nan_equal=False):
    geo = geometry_expected(hits, passes)
    bad = ~same_bits(got[..., 0:3], want_albedo, nan_equal).all(axis=2)
    assert not bad.any(), f"{what}: the albedo of {int(bad.sum())} pixels differs, first at {np.argwhere(bad)[:3].tolist()}"
    assert np.array_equal(got[..., 3:8].view(np.uint32), geo.view(np.uint32)), f"{what}: normal / depth / coverage differ"
    miss = hits[-1]["inst"] < 0 if len(passes) == 1 else np.zeros(got.shape[0:2], bool)
    assert not got[miss].any(), f"{what}: a miss is eight zeros"
