"""The node programs at their numeric edges: every pure node kind (checker, gradient — as a bsdf's operand, which the device evaluates outside the VM, and
inside a program —, blackbody, combine, combineRGB, vecToColor, alpha, grayscale, the 15 math ops, fresnel, rayLength, normal, the 10 vecMath ops) on operands that no fixture holds — zero divisors, negative bases, subnormals, infinities, NaN, signed
zeros, the clamps' boundaries — evaluated by the device VM per hit ("dynamic") and once on the host by the scene compiler ("folded"), and held to a restatement of
the reference's sources (tests/graph_spec.py: Restatement) bit for bit, a NaN equal to a NaN of any payload.

Scenes are copies of nodezoo_display's description (tests/scene_synth.py); every graph is shown as diffuse(colour), so the albedo channel of crh_render_aov reads
it out. A value operand that depends on the hit but is exact is alpha(image(T, NO_BILINEAR)) of a float RGBA texture:
  grids     the textured plane shows combineRGB(op1, op2, op3) of x = alpha(K x 1 texture) and y = alpha(1 x K texture): pixel (u, v) evaluates op(x_i, y_j);
  spheres   a 1 x 1 texture gives one operand for a whole sphere (no nearest fetch on the cube: its uv is (-1, -1)); a vector operand is
            add(C, multiply(normal, (0, 0, 0))) — the restatement follows the same graph;
  packs     the folded counterpart of a grid: combineRGB of three constant graphs per material, 62 materials per scene.

CPU tier: coverage conditions from the oracle's hits, the special classes among the expected values, the restatement pinned to the oracle's render under a white
sky, the compiler's folding and its slot limit, and this file's GPU tests on the kernel emulation. GPU tier: albedo == restatement on every scene, dynamic ==
folded directly, a full-path frame == the oracle's, and the refusal of a program that needs nine operand slots."""
import ctypes as C

import numpy as np
import pytest

from firsthit_spec import fold
from graph_spec import base  # noqa: F401 (the module-scoped fixture: nodezoo_display's scene)
from graph_spec import (CUBE, FLT_MAX, FLT_MIN, INF, NAN, NB, PLANE, SUB_MAX, SUB_MIN, F, ForLibrary, Leaves, Restatement, S, assert_aov, bits, f32, gpu_aov, new_scene, same_bits,
                        scene_hits, size_of, white_sky_selection)
from scene_synth import (COLOR_IMAGE, DIFFUSE, EMISSION, GLASS, METAL, MIX, MATH_ABS, MATH_ADD, MATH_COS, MATH_DIVIDE, MATH_LOG, MATH_MAX, MATH_MIN, MATH_MULTIPLY, MATH_POWER,
                         MATH_SIN, MATH_SQRT, MATH_SUBTRACT, MATH_TAN, MATH_TO_DEGREES, MATH_TO_RADIANS, VEC_ABS, VEC_CROSS, VEC_NORMALIZE, VEC_REFLECT)
from support import ctx, run_gpu_tests_on_emulation  # noqa: F401 (ctx: the fixture)

SLOTS = 8          # CRH_PROG_SLOTS (c-ray_amd/csrc/pt_device.h)


PI = f32(np.pi)
HALF_PI = f32(np.pi / 2)


def neighbours(x):
    return [f32(np.nextafter(F(x), F(-INF))), f32(x), f32(np.nextafter(F(x), F(INF)))]


# the unary ops' operands: 28 columns
UNARY_X = ([0.0, -0.0, SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, INF, -INF, NAN, 0.5, 1.0, 2.0, 10.0, f32(1 / 3), PI]
           + neighbours(HALF_PI) + [f32(2 ** 24), 1e9, 2e38, 128.0, 180.0, 255.0])
# the binary ops' operands, on both axes: both zeros, both infinities, NaN, subnormals, a negative non-integer, odd and even integers of both signs
BINARY_X = [0.0, -0.0, SUB_MIN, -SUB_MAX, FLT_MIN, -FLT_MAX, FLT_MAX, INF, -INF, NAN, 0.5, 1.0, 2.0, 3.0, -2.5, -3.0, -2.0, 10.0, f32(1 / 3), f32(2 ** 24)]
UNARY_OPS = {"log10": MATH_LOG, "sqrt": MATH_SQRT, "abs": MATH_ABS, "sin": MATH_SIN, "cos": MATH_COS, "tan": MATH_TAN, "toRadians": MATH_TO_RADIANS,
             "toDegrees": MATH_TO_DEGREES}
BINARY_OPS = {"add": MATH_ADD, "subtract": MATH_SUBTRACT, "multiply": MATH_MULTIPLY, "divide": MATH_DIVIDE, "power": MATH_POWER, "min": MATH_MIN, "max": MATH_MAX}
# one grid scene holds three ops at once; (name, swapped): swapped is op(y, x)
GRIDS = {"binary add subtract multiply": [("add", False), ("subtract", False), ("multiply", False)],
         "binary divide power min": [("divide", False), ("power", False), ("min", False)],
         "binary max and swapped": [("max", False), ("min", True), ("max", True)],
         "unary log10 sqrt abs": [("log10", False), ("sqrt", False), ("abs", False)],
         "unary sin cos tan": [("sin", False), ("cos", False), ("tan", False)],
         "unary toRadians toDegrees sqrt": [("toRadians", False), ("toDegrees", False), ("sqrt", False)]}
# Every channel of the AOV buffer goes through the frame's running mean, (0 * 0 + sample) * 1 for one pass, which turns a -0 into +0 (and so does the path
# tracer's 0 + weight * sky): the sign of a zero result is not visible in any output as it is. Each grid therefore has a twin that shows 1 / op(x, y): -inf for
# a -0, +inf for a +0 — min(+0, -0) against min(-0, +0), sqrt(-0), 0 * -1, powf(-0, 3).
RECIPROCAL = "1 / "
GRIDS.update({RECIPROCAL + name: [(RECIPROCAL + op, swapped) for op, swapped in ops] for name, ops in list(GRIDS.items())})
BLACKBODY_K = ([0.0, -1000.0, NAN, 1000.0] + neighbours(1900.0) + [1901.0, f32(6599.9995), 6600.0, f32(6600.0005), 6700.0, f32(39999.996), 40000.0, 1e9])
CHECKER_SCALES = [0.0, -0.0, 1.0, 8.0, 1e9, INF, NAN]
FRESNEL_IOR = [-1.0, 0.0, 1.0, 1.45, INF, NAN]
ZERO = (0.0, 0.0, 0.0)
# (a, b) of the vecMath ops. No component is -0: a dynamic vector operand is C + normal * 0, which turns a -0 of C into +0 where the normal's component is positive
VEC_PAIRS = [(ZERO, (1.0, 2.0, 3.0)),                                            # normalize(0) is NaN
             ((FLT_MAX, 0.0, 0.0), (0.5, 0.25, -1.0)),                           # the length overflows inside normalize
             ((1.0, 2.0, 3.0), (2.0, 4.0, 6.0)),                                 # parallel: cross is zero
             ((SUB_MIN, -SUB_MAX, FLT_MIN), (0.5, -0.5, 2.0)),                   # subnormal components, mixed signs
             ((-1.5, 2.25, -3e-3), (4.0, -5.0, 6e10)),
             ((FLT_MAX, -FLT_MAX, 1.0), (FLT_MAX, FLT_MAX, -2.0))]                # sums and products overflow to both infinities
VEC_OP_NAMES = ["add", "subtract", "multiply", "average", "dot", "cross", "normalize", "reflect", "length", "abs"]
WHITE = (1.0, 1.0, 1.0)


def right_deep(s, L, ops, xs):
    """x0 op0 (x1 op1 (... (x[n-1] op[n-1] x[n]))): every level's a operand waits in its slot while the b branch is evaluated: len(ops) + 1 slots."""
    node = L.val(xs[len(ops)])
    for k in reversed(range(len(ops))):
        node = s.math(ops[k], L.val(xs[k]), node)
    return node


def left_deep(s, L, ops, xs):
    """((x0 op0 x1) op1 x2) ...: two slots, and every dst is the slot of its a operand."""
    node = L.val(xs[0])
    for k, op in enumerate(ops):
        node = s.math(op, node, L.val(xs[k + 1]))
    return node


CHAIN_OPS = [MATH_ADD, MATH_MULTIPLY, MATH_SUBTRACT, MATH_DIVIDE, MATH_MAX, MATH_MIN, MATH_POWER]
CHAIN_X = [f32(0.75 + 0.37 * k) for k in range(48)]


def chain_right(s, L, n):
    return s.combine(right_deep(s, L, [CHAIN_OPS[k % 7] for k in range(n)], CHAIN_X))


def chain_left_40(s, L):
    return s.combine(left_deep(s, L, [CHAIN_OPS[k % 6] for k in range(40)], CHAIN_X))


def chain_reuse(s, L):
    """Every dst reuses an operand's slot: unary ops over one slot, then colour / vector / value conversions over the same slots."""
    x = s.math(MATH_SQRT, s.math(MATH_ABS, s.math(MATH_SIN, L.val(2.5), s.value(0.0)), s.value(0.0)), s.value(0.0))
    v = s.vecmath(VEC_ABS, s.vecmath(VEC_NORMALIZE, L.vec(3.0, -4.0, 12.0), s.vec(0.0, 0.0, 0.0)), s.vec(0.0, 0.0, 0.0))
    g = s.grayscale(s.vec_to_color(v))
    return s.combine_rgb(x, g, s.math(MATH_TO_DEGREES, s.math(MATH_TO_RADIANS, s.alpha(s.combine(x)), s.value(0.0)), s.value(0.0)))


# (down, up): negative and > 1 channels, a huge one, alphas that differ
GRADIENT_1 = ((-0.5, 2.0, 0.25, 1.0), (1.5, -1.0, 3.0, 0.5))
GRADIENT_2 = ((4.0, 0.0, -0.0, 0.0), (-3.0, 1e20, 0.5, 2.0))
GRADIENT_OPERANDS = ("gradient", "gradient 2")          # diffuse(gradient): no program


def sphere_graphs():
    """[(label, node kind for the summary's counts, foldable, fn(s, L) -> colour node)]: one sphere each."""
    G = []

    def add(label, kind, foldable, fn):
        G.append((label, kind, foldable, fn))
    for t in BLACKBODY_K:
        add(f"blackbody {t!r}", "blackbody", True, lambda s, L, t=t: s.blackbody(L.val(t)))
    for i in FRESNEL_IOR:
        add(f"fresnel {i!r}", "fresnel", False, lambda s, L, i=i: s.combine(s.fresnel(L.val(i))))
    for sc in CHECKER_SCALES:
        for images in (False, True):
            add(f"checker {sc!r} {'images' if images else 'constants'}", "checker", False, lambda s, L, sc=sc, images=images: checker(s, L, sc, images))
    add("rayLength", "rayLength", False, lambda s, L: s.combine(s.ray_length()))
    add("normal", "normal", False, lambda s, L: s.vec_to_color(s.normal()))
    add("gradient", "gradient", False, lambda s, L: s.gradient(*GRADIENT_1))
    add("gradient 2", "gradient", False, lambda s, L: s.gradient(*GRADIENT_2))
    # a gradient at a bsdf's colour input is an operand kind of its own (scene_compile.cpp: operand), evaluated outside the VM; these three are gradients INSIDE a
    # program: through a checker, which passes the colour on unchanged (scale 8: both branches occur on a sphere), and through alpha and grayscale
    add("checker(gradient, gradient)", "gradient", False, lambda s, L: s.checker(s.gradient(*GRADIENT_1), s.gradient(*GRADIENT_2), L.val(8.0)))
    add("alpha(gradient)", "gradient", False, lambda s, L: s.combine(s.alpha(s.gradient(*GRADIENT_1))))
    add("grayscale(gradient)", "gradient", False, lambda s, L: s.combine(s.grayscale(s.gradient(*GRADIENT_2))))
    add("combine", "combine", True, lambda s, L: s.combine(L.val(0.375)))
    add("vecToColor", "vecToColor", True, lambda s, L: s.vec_to_color(L.vec(0.25, -0.5, 2.0)))
    add("alpha(combine)", "alpha", True, lambda s, L: s.combine(s.alpha(s.combine(L.val(0.3)))))
    add("alpha(vecToColor)", "alpha", True, lambda s, L: s.combine(s.alpha(s.vec_to_color(L.vec(0.25, -0.5, 2.0)))))
    add("alpha(blackbody)", "alpha", True, lambda s, L: s.combine(s.alpha(s.blackbody(L.val(3000.0)))))
    add("grayscale 1e20", "grayscale", True, lambda s, L: s.combine(s.grayscale(s.combine_rgb(L.val(1e20), L.val(0.5), L.val(0.25)))))
    add("grayscale negative", "grayscale", True, lambda s, L: s.combine(s.grayscale(s.combine_rgb(L.val(-0.5), L.val(-2.0), L.val(0.25)))))
    for op, name in enumerate(VEC_OP_NAMES):
        for k, (a, b) in enumerate(VEC_PAIRS):
            add(f"vecMath {name} {k}", "vecMath", True, lambda s, L, op=op, a=a, b=b: s.vec_to_color(s.vecmath(op, L.vec(*a), L.vec(*b))))
    for op in (VEC_REFLECT, VEC_CROSS, VEC_NORMALIZE):
        add(f"vecMath {VEC_OP_NAMES[op]} normal", "vecMath", False, lambda s, L, op=op: s.vec_to_color(s.vecmath(op, s.normal(), L.vec(0.3, -0.6, 0.9))))
    add("chain right 8 slots", "chain", True, lambda s, L: chain_right(s, L, SLOTS - 1))
    add("chain left 40", "chain", True, chain_left_40)
    add("chain reuse", "chain", True, chain_reuse)
    return G


def checker(s, L, scale, images):
    tex = L.textures
    if images:
        a, b = s.image(tex["rgba7x6"], S), s.image(tex["rgbaf2x2"], 0)          # filtered: defined on the cube's uv = (-1, -1) too
    else:
        a, b = s.color(0.8, 0.1, 0.05, 0.25), s.color(0.1, 0.2, 0.9, 0.75)
    return s.checker(a, b, L.val(scale))


GRAPHS = sphere_graphs()
FOLDABLE = [g for g in GRAPHS if g[2]]
# the graphs that read the hit themselves, with constant leaves as well: still programs (or a gradient operand), shown in the dynamic scenes
CONST_LEAF = [(label + " const", kind, False, fn) for label, kind, foldable, fn in GRAPHS if kind in ("fresnel", "checker") or label.endswith(" normal")]
POOL = GRAPHS + CONST_LEAF
# cube and plane of dynamic scene k: the checker's point branch and its uv branch on a mesh. The first N_SPHERE_SCENES of them show the sphere graphs, 60 each
MESH_CHECKERS = [(sc, images) for images in (False, True) for sc in CHECKER_SCALES]
N_DYNAMIC = len(MESH_CHECKERS)
N_SPHERE_SCENES = -(-len(POOL) // 60)


def show(s, labels, entries):
    """entries: [(label, colour node)] -> a material each; spheres cycle through them."""
    for label, node in entries:
        assert label not in labels
        labels[label] = s.material(s.bsdf(DIFFUSE, node))


def build_dynamic(base, k):
    """Dynamic scene k: the cube and the plane show mesh checker k; the spheres of the first N_SPHERE_SCENES scenes show 60 of the sphere graphs each (the last
    of them wraps round to the first graphs), those of the other scenes a plain colour."""
    s, tex = new_scene(base, "spheres")
    L, Lc = Leaves(s, True, tex), Leaves(s, False, tex)
    labels = {}
    if k < N_SPHERE_SCENES:
        chosen = [POOL[(60 * k + i) % len(POOL)] for i in range(60)]
        show(s, labels, [(g[0], g[3](s, Lc if g in CONST_LEAF else L)) for g in chosen])
        names = [g[0] for g in chosen]
    else:
        show(s, labels, [("other", s.color(0.5, 0.5, 0.5))])
        names = ["other"] * 60
    for i in range(60):
        s.set_sphere_material(i, labels[names[i]])
    sc, images = MESH_CHECKERS[k]
    show(s, labels, [("cube", checker(s, Lc, sc, images)), ("plane", checker(s, L, sc, images))])          # (no nearest fetch on the cube: its scale is a constant)
    s.set_mesh_material(CUBE, labels["cube"])
    s.set_mesh_material(PLANE, labels["plane"])
    return s, labels


def op_code(name):
    return BINARY_OPS[name] if name in BINARY_OPS else UNARY_OPS[name]


def pack_cases():
    """Every (op, x, y) of the grids as a constant graph: [(op name, x, y)], three per material; and 1 / op(x, y) where the reference's op(x, y) is a zero."""
    cases = [(name, x, y) for name in BINARY_OPS for x in BINARY_X for y in BINARY_X]
    cases += [(name, x, 0.0) for name in UNARY_OPS for x in UNARY_X]
    return cases + [(RECIPROCAL + name, x, y) for name, x, y in cases if Restatement.math(op_code(name), F([x]), F([y]))[0] == 0]


PACK = pack_cases()
PER_SCENE = 62 * 3
N_FOLDED_SPHERES = -(-len(FOLDABLE) // 60)
N_PACKS = -(-len(PACK) // PER_SCENE)


def op_node(s, name, x, y):
    if name.startswith(RECIPROCAL):
        return s.math(MATH_DIVIDE, s.value(1.0), op_node(s, name[len(RECIPROCAL):], x, y))
    return s.math(op_code(name), x, y)


def build_folded(base, k):
    """Folded scene k < N_FOLDED_SPHERES: the foldable sphere graphs with constant leaves. After those: pack k - N_FOLDED_SPHERES of the grids' cases."""
    s, tex = new_scene(base, "spheres")
    L = Leaves(s, False, tex)
    labels = {}
    if k < N_FOLDED_SPHERES:
        chosen = [FOLDABLE[(60 * k + i) % len(FOLDABLE)] for i in range(60)]
        show(s, labels, [(g[0], g[3](s, L)) for g in chosen] + [("cube", s.color(0.5, 0.5, 0.5)), ("plane", s.color(0.25, 0.5, 0.75))])
        names = [g[0] for g in chosen]
    else:
        cases = PACK[(k - N_FOLDED_SPHERES) * PER_SCENE:][:PER_SCENE]
        cases = cases + cases[:(-len(cases)) % 3]
        names = []
        for m in range(0, len(cases), 3):
            label = f"pack {k} {m // 3}"
            show(s, labels, [(label, s.combine_rgb(*[op_node(s, n, s.value(x), s.value(y)) for n, x, y in cases[m:m + 3]]))])
            labels[label + " cases"] = cases[m:m + 3]
            names.append(label)
        while len(names) < 62:
            names.append(names[len(names) % (len(cases) // 3)])
        labels["cube"], labels["plane"] = labels[names[60]], labels[names[61]]
    for i in range(60):
        s.set_sphere_material(i, labels[names[i]])
    s.set_mesh_material(CUBE, labels["cube"])
    s.set_mesh_material(PLANE, labels["plane"])
    return s, labels


def grid_textures(xs, ys):
    """K x 1: x in the alpha by column; 1 x K: y in the alpha by row."""
    tx = np.zeros((1, len(xs), 4), F)
    tx[0, :, 3] = F(xs)
    ty = np.zeros((len(ys), 1, 4), F)
    ty[:, 0, 3] = F(ys)
    return tx, ty


def build_grid(base, name):
    """The plane shows combineRGB of three ops of (x_i, y_j); the spheres and the cube a plain colour."""
    s, _ = new_scene(base, "mesh")
    ops = GRIDS[name]
    binary = ops[0][0].replace(RECIPROCAL, "") in BINARY_OPS
    xs = BINARY_X if binary else UNARY_X
    ys = BINARY_X if binary else [0.0]
    ptx, pty = grid_textures(xs, ys)
    tx, ty = s.texture(ptx), s.texture(pty)
    labels = {}

    def channel(op, swapped):
        x, y = s.alpha(s.image(tx, NB)), s.alpha(s.image(ty, NB))
        return op_node(s, op, y, x) if swapped else op_node(s, op, x, y)
    show(s, labels, [("plane", s.combine_rgb(*[channel(*o) for o in ops])), ("other", s.color(0.5, 0.5, 0.5))])
    for i in range(60):
        s.set_sphere_material(i, labels["other"])
    s.set_mesh_material(CUBE, labels["other"])
    s.set_mesh_material(PLANE, labels["plane"])
    labels["grid"] = {"tx": tx, "ty": ty, "xs": xs, "ys": ys}
    return s, labels


BUILDERS = {"dynamic": build_dynamic, "folded": build_folded, "grid": build_grid}
SCENES = ([("dynamic", k) for k in range(N_DYNAMIC)] + [("folded", k) for k in range(N_FOLDED_SPHERES + N_PACKS)] + [("grid", n) for n in GRIDS])


_cases = {}


def view_of(kind):
    return "mesh" if kind == "grid" else "spheres"


def cpu_case(oracle, base, kind, key):
    """(scene, labels, pass-0 hits with directions, expected albedo): computed once, shared, left unchanged."""
    if (kind, key) not in _cases:
        s, labels = BUILDERS[kind](base, key)
        hits = scene_hits(oracle, s, view_of(kind), dirs=True)[0]
        want = Restatement(s.desc).frame(hits)
        _cases[kind, key] = (s, labels, hits, want)
    return _cases[kind, key]


def in_the_buffer(want):
    """What one pass leaves in the AOV buffer (and the path tracer in the frame): the running mean of renderer.c:288-291 from zeros, which is the sample but for
    a -0, which it turns into +0."""
    return fold(np.zeros_like(want), want, 1)


def material_pixels(labels, hits, label):
    return (hits["inst"] >= 0) & (hits["material"] == labels[label])


def grid_cells(s, labels, hits):
    """(plane pixels, column index, row index): the texel of each operand texture that the restatement's nearest fetch reads at every plane pixel."""
    sel = material_pixels(labels, hits, "plane")
    g = labels["grid"]
    r = Restatement(s.desc)
    d = s.desc
    images = [j for j in range(d.gnode_count) if d.gnodes[j].kind == COLOR_IMAGE and d.gnodes[j].b == NB]
    r.color(next(j for j in images if d.gnodes[j].a == g["tx"]), hits[sel])
    r.color(next(j for j in images if d.gnodes[j].a == g["ty"]), hits[sel])
    assert r.probes[0]["height"] == 1 and r.probes[1]["width"] == 1
    # the stored row of y is height - 1 - y (texture.c:39): the operand of texel row ty is ys[K - 1 - ty]
    return sel, r.probes[0]["tx"], len(g["ys"]) - 1 - r.probes[1]["ty"]


def unique_rows(a):
    return np.unique(np.ascontiguousarray(a, F).view(np.uint32).reshape(-1, a.shape[-1]), axis=0)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def special_classes(values):
    v = np.asarray(values, F).reshape(-1)
    b = v.view(np.uint32)
    return {"nan": int(np.isnan(v).sum()), "+inf": int((v == INF).sum()), "-inf": int((v == -INF).sum()), "-0": int((b == 0x80000000).sum()),
            "subnormal": int(((v != 0) & (np.abs(v) < F(FLT_MIN))).sum())}


@pytest.mark.parametrize("name", list(GRIDS))
def test_every_cell_of_a_grid_is_seen(name, oracle, base):
    """Conditions, not measurements: from the oracle's hits, every (x_i, y_j) cell shows at least 4 pixels of the plane, and the expected values of the grid
    hold every special class the ops can give."""
    s, labels, hits, want = cpu_case(oracle, base, "grid", name)
    sel, ci, cj = grid_cells(s, labels, hits)
    K, Ky = len(labels["grid"]["xs"]), len(labels["grid"]["ys"])
    counts = np.zeros((Ky, K), int)
    np.add.at(counts, (cj, ci), 1)
    got = special_classes(want[sel])
    print(f"{name}: {int(sel.sum())} plane pixels, {K} x {Ky} cells, fewest pixels in a cell {counts.min()}, most {counts.max()}; expected values: {got}")
    assert counts.min() >= 4, counts
    if name.startswith(RECIPROCAL):          # both signs of a zero result occur, as the two infinities
        need = ["nan", "+inf", "-inf"]
    else:
        need = ["nan", "-0", "subnormal"] if name == "unary sin cos tan" else ["nan", "+inf", "-inf", "-0", "subnormal"]
    for c in need:
        assert got[c] >= 4, (name, c, got)
    # every cell's pixels expect one value: the operands are exact
    for j in range(Ky):
        for i in range(K):
            assert len(unique_rows(want[sel][(ci == i) & (cj == j)])) == 1, (name, i, j)


def test_min_and_max_meet_pairs_where_the_order_of_the_operands_decides(oracle, base):
    """min / max are the reference's macros: on (+0, -0), (-0, +0) and on a NaN with a number the result is the SECOND operand, or depends on which is which.
    The grid holds those pairs, and the expectation differs between min(x, y) and min(y, x) there."""
    s, labels, hits, want = cpu_case(oracle, base, "grid", "binary max and swapped")
    sel, ci, cj = grid_cells(s, labels, hits)
    w = want[sel]
    mn = cpu_case(oracle, base, "grid", "binary divide power min")[3][sel][:, 2]          # min(x, y); this scene: max(x, y), min(y, x), max(y, x)
    order = ~same_bits(mn, w[:, 1], nan_equal=True)
    cells = {(int(i), int(j)) for i, j in zip(ci[order], cj[order])}
    xs = labels["grid"]["xs"]
    zero_pairs = [(i, j) for i, j in cells if xs[i] == 0 and xs[j] == 0]
    nan_pairs = [(i, j) for i, j in cells if np.isnan(xs[i]) != np.isnan(xs[j])]
    print(f"min(x, y) != min(y, x) in {len(cells)} cells: {len(zero_pairs)} of signed zeros, {len(nan_pairs)} of a NaN and a number")
    assert len(zero_pairs) == 2 and len(nan_pairs) == 2 * (len(xs) - 1) and len(cells) == len(zero_pairs) + len(nan_pairs)
    assert not same_bits(w[:, 0], w[:, 2], nan_equal=True)[order].any()          # and so does max
    # ... and the reciprocal twins carry the signed-zero pairs into the buffer: -inf against +inf
    r = in_the_buffer(cpu_case(oracle, base, "grid", RECIPROCAL + "binary max and swapped")[3])[sel]
    rmn = in_the_buffer(cpu_case(oracle, base, "grid", RECIPROCAL + "binary divide power min")[3])[sel][:, 2]
    zeros = np.isin(ci, [i for i, x in enumerate(xs) if x == 0]) & np.isin(cj, [i for i, x in enumerate(xs) if x == 0]) & (ci != cj)
    assert zeros.sum() >= 8 and np.isinf(rmn[zeros]).all() and (rmn[zeros] == -r[zeros, 1]).all() and (r[zeros, 0] == -r[zeros, 2]).all()


def test_every_sphere_graph_is_seen(oracle, base):
    """Every graph of every dynamic and folded scene shows at least 30 hit pixels; every graph is in a scene; the special classes occur among the expectations."""
    seen, classes = set(), {}
    for kind, key in SCENES:
        if kind == "grid":
            continue
        s, labels, hits, want = cpu_case(oracle, base, kind, key)
        counts = {label: int(material_pixels(labels, hits, label).sum()) for label, m in labels.items() if isinstance(m, int)}
        low = {k: v for k, v in counts.items() if v < 30}
        print(kind, key, "fewest pixels of a graph:", min(counts.values()))
        assert not low, (kind, key, low)
        seen |= {(kind, label) for label in counts}
        for k, v in special_classes(want[hits["inst"] >= 0]).items():
            classes[kind, k] = classes.get((kind, k), 0) + v
    print(classes)
    for g in POOL:
        assert ("dynamic", g[0]) in seen, g[0]
    for g in FOLDABLE:
        assert ("folded", g[0]) in seen, g[0]
    for kind in ("dynamic", "folded"):
        for c in ("nan", "+inf", "-inf", "-0", "subnormal"):
            assert classes[kind, c] >= 30, (kind, c, classes)


_escaped = {}


def escaped(oracle, base, view):
    """Where the second ray of the oracle's 1-sample, 2-bounce render leaves the scene: the render of the same geometry with every surface diffuse white under a
    white sky (a diffuse node's scattered direction depends on the normal and the sampler alone, not on its colour)."""
    if view not in _escaped:
        s, _ = new_scene(base, view)
        m = s.material(s.bsdf(DIFFUSE, s.color(*WHITE)))
        for i in range(60):
            s.set_sphere_material(i, m)
        s.set_mesh_material(CUBE, m)
        s.set_mesh_material(PLANE, m)
        s.white_sky()
        w, h = size_of(view)
        _escaped[view] = (oracle.render(s, w, h, 1, 2, threads=1)[0] != 0).any(axis=2)
    return _escaped[view]


@pytest.mark.parametrize("kind", ["dynamic", "folded", "grid"])
def test_restatement_equals_the_oracles_render_under_a_white_sky(kind, oracle, base):
    """The restatement pinned to the oracle on every scene: where the first hit is a diffuse root and the second ray escaped, the pixel of the 1-sample, 2-bounce
    frame under a white sky is the albedo. Bits, a NaN equal to any NaN.

    What the oracle's path code (pathtrace.c:32-60, renderer.c:288-291) does to an albedo on the way, and what is done about it here:
      -0        the frame is 0 + weight * sky and then (0 * 0 + sample) * 1: a -0 channel arrives as +0, as it does in the AOV buffer (`in_the_buffer`); the
                reciprocal grids and packs show the sign of a zero result as the sign of an infinity;
      non-finite where the second ray did NOT escape, the second hit's emission 0 is multiplied by the weight: inf * 0 = NaN, and a pixel with a NaN channel is black
                in its other channels but not black as a whole, so white_sky_selection selects it. Pixels whose expectation has a non-finite channel are
                therefore compared only where the second ray escaped in the render of the same geometry with white diffuse surfaces (`escaped`);
      black     an albedo of (0, 0, 0) — vecMath's dot and length, alpha(vecToColor) — gives a black pixel wherever the second ray went, which the selection
                drops: those materials are compared on ALL their pixels instead (with zeros), and the half-of-the-pixels condition does not apply to them.
    Negative, huge and subnormal channels arrive unchanged. The GPU tier holds nothing out."""
    for k, key in [sc for sc in SCENES if sc[0] == kind]:
        _, labels, hits, want = cpu_case(oracle, base, kind, key)
        view = view_of(kind)
        s, _ = BUILDERS[kind](base, key)          # (a copy of its own: the shared case keeps its sky)
        img, sel = white_sky_selection(oracle, s, hits, view)
        finite = np.isfinite(want).all(axis=2)
        sel = sel & (finite | escaped(oracle, base, view))
        hit = hits["inst"] >= 0
        black = hit & (want == 0).all(axis=2)
        for label, m in labels.items():
            if not isinstance(m, int):
                continue
            here = hit & (hits["material"] == m)
            if kind == "grid" and label == "plane":
                ok = 2 * (sel & here).sum() >= here.sum()          # (cells of black or non-finite values are part of the plane's pixels)
            else:
                ok = 2 * (sel & here & ~black).sum() >= (here & ~black).sum()
            assert ok, (kind, key, label, int((sel & here).sum()), int(here.sum()))
        check = sel | black
        if kind == "grid":          # the hold-out's extent as a condition: every cell of the grid, the non-finite ones included, is compared with the oracle
            plane, ci, cj = grid_cells(cpu_case(oracle, base, kind, key)[0], labels, hits)
            compared = np.zeros((len(labels["grid"]["ys"]), len(labels["grid"]["xs"])), int)
            np.add.at(compared, (cj, ci), check[plane].astype(int))
            print(f"{kind} {key}: fewest compared pixels in a cell {compared.min()}")
            assert compared.min() >= 1, compared
        plus0 = in_the_buffer(want)
        bad = ~same_bits(img[check], plus0[check], nan_equal=True).all(axis=1)
        print(f"{kind} {key}: {int(check.sum())} of {int(hit.sum())} hit pixels compared")
        assert not bad.any(), (kind, key, int(bad.sum()), img[check][bad][:3], want[check][bad][:3], np.argwhere(check)[bad][:3])


def prog_ops(emu, s):
    n = C.c_uint32()
    rc = emu.emu_compile_check(s.ptr, None, C.byref(n), None)
    return rc, n.value


def test_the_compiler_folds_constant_graphs_and_keeps_dynamic_ones(emu, oracle, base):
    """Through the scene compiler built for the host: a folded scene's graphs produce no program op beyond those of the fixture's own (unshown) graphs; every
    dynamic graph adds at least one program."""
    plain, _ = new_scene(base, "spheres")
    rc, floor = prog_ops(emu, plain)
    assert rc == 0, emu.emu_last_error()
    for k in range(N_FOLDED_SPHERES + N_PACKS):
        rc, n = prog_ops(emu, cpu_case(oracle, base, "folded", k)[0])
        assert rc == 0 and n == floor, ("folded", k, n, floor, emu.emu_last_error())
    s, tex = new_scene(base, "spheres")
    L, Lc = Leaves(s, True, tex), Leaves(s, False, tex)
    before = floor
    for g in POOL:
        if g[0] in GRADIENT_OPERANDS:          # a gradient at a bsdf's colour input is an operand kind of its own, not a program (scene_compile.cpp: operand)
            s.material(s.bsdf(DIFFUSE, g[3](s, L)))
            rc, n = prog_ops(emu, s)
            assert rc == 0 and n == before, (g[0], n, before, emu.emu_last_error())
            continue
        s.material(s.bsdf(DIFFUSE, g[3](s, Lc if g in CONST_LEAF else L)))
        rc, n = prog_ops(emu, s)
        assert rc == 0 and n >= before + 2, (g[0], n, before, emu.emu_last_error())          # at least one op and the end marker
        before = n
    for name in GRIDS:
        rc, n = prog_ops(emu, cpu_case(oracle, base, "grid", name)[0])
        assert rc == 0 and n >= floor + 2 * 3 + 2, (name, n, floor)


def nine_slot_scene(base, dynamic):
    s, tex = new_scene(base, "spheres")
    L = Leaves(s, dynamic)
    m = s.material(s.bsdf(DIFFUSE, chain_right(s, L, SLOTS)))
    for i in range(60):
        s.set_sphere_material(i, m)
    return s


@pytest.mark.parametrize("dynamic", [True, False])
def test_a_program_of_nine_slots_is_refused_by_the_compiler(dynamic, emu, oracle, base):
    """A right-deep chain of 8 math ops needs 9 operand slots: CRH_ERR_UNSUPPORTED with the slot message — as a program, and when the compiler folds it (the
    fold runs the same program on the host). The chain of 7 ops, 8 slots, is accepted (it is in the dynamic and the folded scenes)."""
    rc, _ = prog_ops(emu, nine_slot_scene(base, dynamic))
    assert rc == oracle.abi.ERR_UNSUPPORTED, rc
    assert "CRH_PROG_SLOTS" in emu.emu_last_error().decode(), emu.emu_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------------------------------------
_albedo = {}


def device_albedo(pkg, ctx, oracle, base, kind, key):
    """The AOV buffer of one pass of a scene, rendered once and shared by the tests that read it."""
    if (kind, key) not in _albedo:
        s = cpu_case(oracle, base, kind, key)[0]
        w, h = size_of(view_of(kind))
        _albedo[kind, key] = gpu_aov(pkg, ctx, s, w, h, 1)
    return _albedo[kind, key]


GROUPS = {"dynamic spheres": [("dynamic", k) for k in range(N_SPHERE_SCENES)], "dynamic mesh checkers": [("dynamic", k) for k in range(N_SPHERE_SCENES, N_DYNAMIC)],
          "folded": [sc for sc in SCENES if sc[0] == "folded"], "grids": [sc for sc in SCENES if sc[0] == "grid"]}


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_albedo_equals_the_restatement(group, pkg, ctx, oracle, base):
    """One pass of one on every scene, dynamic and folded: every hit pixel's albedo bit for bit (a NaN equal to any NaN), a miss's eight zeros, the geometry
    channels."""
    for kind, key in GROUPS[group]:
        _, _, hits, want = cpu_case(oracle, base, kind, key)
        got = device_albedo(pkg, ctx, oracle, base, kind, key)
        assert (hits["inst"] >= 0).sum() >= 2000
        assert_aov(got, in_the_buffer(want), hits[None], [0], f"{kind} {key}", nan_equal=True)


def one_value(got, sel, what):
    px = got[sel][:, 0:3]
    assert len(px) and same_bits(px, px[0][None], nan_equal=True).all(), f"{what}: a constant graph gives more than one albedo: {unique_rows(px).view(F)[:4]}"
    return px[0]


@pytest.mark.gpu
def test_dynamic_albedo_equals_folded_albedo(pkg, ctx, oracle, base):
    """The device VM per hit against the scene compiler's fold on the host, directly: every foldable sphere graph, and every cell of every grid against the
    constant graph of the same op and operands in the packs."""
    folded = {}
    for k in range(N_FOLDED_SPHERES + N_PACKS):
        _, labels, hits, _ = cpu_case(oracle, base, "folded", k)
        got = device_albedo(pkg, ctx, oracle, base, "folded", k)
        for label, m in labels.items():
            if isinstance(m, int) and label not in ("cube", "plane"):
                v = one_value(got, material_pixels(labels, hits, label), f"folded {label}")
                for c, case in enumerate(labels.get(label + " cases", [])):
                    folded[case[0], bits(case[1]), bits(case[2])] = v[c]
                if not label.startswith("pack"):
                    folded[label] = v
    compared = 0
    for k in range(N_DYNAMIC):
        _, labels, hits, _ = cpu_case(oracle, base, "dynamic", k)
        got = device_albedo(pkg, ctx, oracle, base, "dynamic", k)
        for g in FOLDABLE:
            if g[0] in labels:
                sel = material_pixels(labels, hits, g[0])
                bad = ~same_bits(got[sel][:, 0:3], folded[g[0]][None], nan_equal=True).all(axis=1)
                assert not bad.any(), f"{g[0]}: the device gives {got[sel][bad][0, 0:3]} per hit, the compiler's fold {folded[g[0]]}"
                compared += 1
    assert compared >= len(FOLDABLE)
    for name, ops in GRIDS.items():
        s, labels, hits, _ = cpu_case(oracle, base, "grid", name)
        got = device_albedo(pkg, ctx, oracle, base, "grid", name)
        sel, ci, cj = grid_cells(s, labels, hits)
        xs, ys = labels["grid"]["xs"], labels["grid"]["ys"]
        px = got[sel]
        for c, (op, swapped) in enumerate(ops):
            keys = [[(op, bits(ys[j]), bits(xs[i])) if swapped else (op, bits(xs[i]), bits(ys[j])) for i in range(len(xs))] for j in range(len(ys))]
            packed = np.array([[k in folded for k in row] for row in keys])          # (a reciprocal is in the packs where op(x, y) is a zero)
            assert packed.all() or op.startswith(RECIPROCAL)          # (cos gives no zero on these operands)
            table = np.array([[folded.get(k, NAN) for k in row] for row in keys], F)
            bad = ~same_bits(px[:, c], table[cj, ci], nan_equal=True) & packed[cj, ci]
            first = np.argwhere(bad)[:1].reshape(-1)
            assert not bad.any(), (f"{name}: {op}{' swapped' if swapped else ''}: {int(bad.sum())} pixels: the device gives "
                                   f"{px[first, c]} per hit for x = {F(xs)[ci[first]]}, y = {F(ys)[cj[first]]}, the compiler's fold {table[cj, ci][first]}")


def build_render_scene(base):
    """Finite operands only; node programs also drive metal roughness, glass roughness and IOR, the mix factor and emission strength."""
    s, tex = new_scene(base, "spheres")
    L, Lc = Leaves(s, True, tex), Leaves(s, False, tex)
    D = lambda c: s.bsdf(DIFFUSE, c)          # noqa: E731
    mats = [
        s.bsdf(METAL, s.blackbody(L.val(4500.0)), s.math(MATH_MULTIPLY, L.val(0.5), s.math(MATH_ABS, s.math(MATH_SIN, s.ray_length(), s.value(0.0)), s.value(0.0)))),
        s.bsdf(GLASS, s.color(0.9, 0.95, 1.0), s.math(MATH_MIN, L.val(0.08), s.fresnel(L.val(1.3))), s.math(MATH_ADD, L.val(1.0), s.math(MATH_DIVIDE, L.val(0.9), L.val(2.0)))),
        s.bsdf(MIX, D(s.color(0.9, 0.2, 0.1)), D(checker(s, L, 8.0, True)), s.fresnel(L.val(1.45))),
        s.bsdf(MIX, D(s.vec_to_color(s.vecmath(VEC_ABS, s.normal(), s.vec(0.0, 0.0, 0.0)))), s.bsdf(METAL, s.color(0.8, 0.8, 0.8), L.val(0.1)),
               s.math(MATH_POWER, s.math(MATH_COS, s.math(MATH_TO_RADIANS, L.val(60.0), s.value(0.0)), s.value(0.0)), L.val(2.0))),
        s.bsdf(EMISSION, s.gradient((0.2, 0.3, 0.9, 1.0), (1.0, 0.8, 0.3, 1.0)), s.math(MATH_MAX, L.val(0.5), s.math(MATH_LOG, s.math(MATH_MULTIPLY, s.ray_length(), L.val(40.0)), s.value(0.0)))),
        D(s.combine_rgb(s.math(MATH_SQRT, L.val(0.3), s.value(0.0)), s.math(MATH_SUBTRACT, L.val(1.0), s.fresnel(L.val(1.8))), s.grayscale(checker(s, L, 1.0, False)))),
        D(s.combine(s.math(MATH_TO_DEGREES, s.math(MATH_TAN, L.val(0.004), s.value(0.0)), s.value(0.0)))),
        D(chain_left_40(s, L)),
    ]
    ids = [s.material(b) for b in mats]
    for i in range(60):
        s.set_sphere_material(i, ids[i % len(ids)])
    s.set_mesh_material(CUBE, s.material(D(checker(s, Lc, 8.0, False))))
    s.set_mesh_material(PLANE, s.material(D(checker(s, L, 8.0, True))))
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("halton", [False, True], ids=["random", "halton"])
def test_frame_equals_the_oracles(halton, pkg, ctx, oracle, base):
    """crh_render_region at 4 samples and 6 bounces against oracle.render of the same description: the frame bit for bit, and the ray count."""
    s = build_render_scene(base)
    w, h = size_of("spheres")
    want, ocnt = oracle.render(s, w, h, 4, 6, halton=halton, threads=1 if halton else 0)
    ctx.set_option(pkg.abi.OPT_SAMPLER, pkg.abi.SAMPLER_HALTON if halton else pkg.abi.SAMPLER_RANDOM)
    try:
        ctx.upload(ForLibrary(pkg, s))
        fb = ctx.framebuffer(w, h)
        ctx.reset_counters()
        ctx.render_region(fb, w, h, 4, 6)
        got = ctx.download(fb, w, h)
        rays = ctx.counters()["rays"]
    finally:
        ctx.set_option(pkg.abi.OPT_SAMPLER, pkg.abi.SAMPLER_RANDOM)
    assert want.any() and np.isfinite(want).all()
    assert rays == ocnt["rays"]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} floats differ"


@pytest.mark.gpu
@pytest.mark.parametrize("dynamic", [True, False], ids=["dynamic", "folded"])
def test_a_program_of_nine_slots_is_refused_at_upload(dynamic, pkg, ctx, oracle, base):
    """crh_scene_upload answers CRH_ERR_UNSUPPORTED with the slot message; the scene with the 8-slot chain on the same context then gives its albedo again."""
    with pytest.raises(pkg.api.CrhError) as e:
        ctx.upload(ForLibrary(pkg, nine_slot_scene(base, dynamic)))
    assert e.value.code == pkg.abi.ERR_UNSUPPORTED, str(e.value)
    assert "CRH_PROG_SLOTS" in str(e.value), str(e.value)
    kind, key = next((k, i) for k, i in SCENES if k == ("dynamic" if dynamic else "folded") and "chain right 8 slots" in cpu_case(oracle, base, k, i)[1])
    s, _, hits, want = cpu_case(oracle, base, kind, key)
    w, h = size_of("spheres")
    assert_aov(gpu_aov(pkg, ctx, s, w, h, 1), in_the_buffer(want), hits[None], [0], "the 8-slot scene after the refused one", nan_equal=True)


N_GPU_TESTS = len(GROUPS) + 1 + 2 + 2


def test_node_edges_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the kernel emulation (tests/emu/libcray_hip_emu.so: k_aov, the render kernels and the scene
    compiler compiled unmodified on the HIP-on-CPU shim) — every one of them runs and passes there, none skipped."""
    run_gpu_tests_on_emulation(__file__, N_GPU_TESTS)
