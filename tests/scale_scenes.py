"""Scaled, shifted and far-viewed versions of the fuzz and KAT scenes, and far-origin ray sets,
shared by tests/test_scale_oracle.py (CPU) and tests/test_scale_gpu.py (GPU).

Every scene is a definition tuple (meshes, lights, cam_def, background, ambience, max_depth) as
fuzz_scenes.scene and kat_scenes.scenes give it, mapped by x -> s * x + t on every vertex, light
position, eye and centre (up, fovy, materials and depth stay), rebuilt as minirt.Mesh objects,
written with minirt.write_sce and read back through the product loader (rt_host_load): the oracle,
minirt and the device all see the same doubles.

Loaded scenes, their oracles and the oracle's frames are computed once per key and shared; callers
must not modify them."""
import math
import tempfile
from pathlib import Path

import numpy as np

import fuzz_scenes
import kat_scenes
import minirt
import pyoracle
import query_cases as qc
import rtamd

REF, ORD = pyoracle.MODE_REFERENCE, pyoracle.MODE_ORDERED
ZERO = (0.0, 0.0, 0.0)

# name -> (s, t): the one table of the CPU and the GPU tests
TRANSFORMS = {
    "identity": (1.0, ZERO),
    "x2^10": (2.0 ** 10, ZERO),
    "x2^-10": (2.0 ** -10, ZERO),
    "x1000": (1000.0, ZERO),
    "x1e-3": (1e-3, ZERO),
    "x2^20": (2.0 ** 20, ZERO),
    "x2^-14": (2.0 ** -14, ZERO),
    "x2^-16": (2.0 ** -16, ZERO),
    "x2^-20": (2.0 ** -20, ZERO),
    "shift1e3": (1.0, (1000.0, -2000.0, 500.0)),
    "shift1e6": (1.0, (1e6, 1e6, -1e6)),
    "x1e4+3e5": (1e4, (3e5, 0.0, 0.0)),
}
# the four at which the oracle is also held against minirt's brute force, and the KAT scenes run
BRUTE_TRANSFORMS = ("identity", "x2^10", "x2^-10", "shift1e3")
KAT_NAMES = ("mirror", "shadow", "phong")
SEEDS = range(8)
VARIANT_SEEDS = range(4)
W, H = 32, 24

# name -> (function, value): far lights, far eyes and a stray vertex on the unit-scale seed scene
VARIANTS = {
    "outlier1e6": ("outlier", 1e6), "outlier1e12": ("outlier", 1e12),
    "sun1e3": ("sun", 1e3), "sun1e6": ("sun", 1e6),
    "telephoto1e2": ("telephoto", 1e2), "telephoto1e4": ("telephoto", 1e4),
}
# rendered by the oracle alone: the largest coordinate upload takes (RT_MAX_COORDINATE) and one
# beyond the supported range (rt_hip.h, rt_scene_upload), where upload refuses the scene
CPU_ONLY_VARIANTS = {"outlier2^61": ("outlier", 2.0 ** 61), "outlier1e30": ("outlier", 1e30)}

# Non-vacuity of the inputs, asserted on the oracle's own counts (conditions, not measurements):
# summed over SEEDS, closest_hits / (primary + reflection rays) is 0.35-0.39 from x2^-16 up to
# x2^20; at x2^-16 ordinary triangles fall below |S| < 1e-10, so the fraction is strictly below the
# identity's; at x2^-20 every triangle does, so nothing is hit and no shadow ray is cast.
MIN_HIT_FRACTION = 0.25
ALL_REJECTED = "x2^-20"
PARTLY_REJECTED = "x2^-16"

# seed 0 at this scale has max|vertex| = 3.2 * 2^59 = 1.8e18: the top of the supported range
TOP_SCALE = 2.0 ** 59

FAR_FLAVOURS = ("vertex", "axis", "tmax")
FAR_FACTORS = (1e2, 1e4, 2.0 ** 20)
FAR_SCENES = ("cornell", "office")


def spp_of(seed):
    """Samples per axis of a seed's frame, as the fuzz tests choose it."""
    return 2 if seed % 4 == 3 else 1


def _map(v, s, t):
    return tuple(s * float(v[k]) + t[k] for k in range(3))


def transform_def(defn, s, t):
    """The definition with x -> s * x + t applied to every position."""
    meshes, lights, cam, bg, amb, depth = defn
    eye, center, up, fovy, w, h = cam
    out_meshes = [minirt.Mesh([_map(v, s, t) for v in m.verts], m.tris, m.mode, m.mat) for m in meshes]
    out_lights = [(_map(lp, s, t), lc) for lp, lc in lights]
    return out_meshes, out_lights, (_map(eye, s, t), _map(center, s, t), up, fovy, w, h), bg, amb, depth


def transformed(seed, s, t, width=W, height=H):
    """fuzz_scenes.scene(seed, width, height) under x -> s * x + t."""
    return transform_def(fuzz_scenes.scene(seed, width, height), s, t)


def transformed_kat(name, s, t):
    """The KAT scene `name` (its own 9 x 7 camera) under x -> s * x + t."""
    return transform_def(kat_scenes.scenes()[name], s, t)


def _box(meshes):
    """(lo, hi, centre, diagonal) of the vertices' box."""
    vs = [v for m in meshes for v in m.verts]
    lo = tuple(min(v[k] for v in vs) for k in range(3))
    hi = tuple(max(v[k] for v in vs) for k in range(3))
    c = tuple(0.5 * (lo[k] + hi[k]) for k in range(3))
    return lo, hi, c, math.sqrt(sum((hi[k] - lo[k]) ** 2 for k in range(3)))


def outlier(seed, value, width=W, height=H):
    """The seed's scene with the x of mesh 1's first vertex replaced by `value`."""
    meshes, lights, cam, bg, amb, depth = fuzz_scenes.scene(seed, width, height)
    m = meshes[1]
    verts = [(float(value), m.verts[0][1], m.verts[0][2])] + m.verts[1:]
    meshes[1] = minirt.Mesh(verts, m.tris, m.mode, m.mat)
    return meshes, lights, cam, bg, amb, depth


def sun(seed, factor, width=W, height=H):
    """The seed's scene with light 0 moved to `factor` root-box diagonals from the box's centre,
    along its own direction from there."""
    meshes, lights, cam, bg, amb, depth = fuzz_scenes.scene(seed, width, height)
    _, _, c, diag = _box(meshes)
    u = minirt.normalize(minirt.sub(lights[0][0], c))
    lights[0] = (tuple(c[k] + factor * diag * u[k] for k in range(3)), lights[0][1])
    return meshes, lights, cam, bg, amb, depth


def telephoto(seed, factor, width=W, height=H):
    """The seed's scene seen from `factor` root-box diagonals further back along the view
    direction, fovy narrowed so that the image plane (through the centre) covers the same region."""
    meshes, lights, cam, bg, amb, depth = fuzz_scenes.scene(seed, width, height)
    eye, center, up, fovy, w, h = cam
    _, _, _, diag = _box(meshes)
    view = minirt.sub(center, eye)
    dist = math.sqrt(minirt.dot(view, view))
    view = minirt.normalize(view)
    far = dist + factor * diag
    new_eye = tuple(center[k] - far * view[k] for k in range(3))
    new_fovy = 2.0 * math.atan(dist * math.tan(0.5 * fovy / 180.0 * math.pi) / far) * 180.0 / math.pi
    return meshes, lights, (new_eye, center, up, new_fovy, w, h), bg, amb, depth


def variant(name, seed):
    fn, value = {**VARIANTS, **CPU_ONLY_VARIANTS}[name]
    return {"outlier": outlier, "sun": sun, "telephoto": telephoto}[fn](seed, value)


def mini(defn):
    """The definition as a minirt.Scene (brute force)."""
    meshes, lights, cam, bg, amb, depth = defn
    eye, center, up, fovy, w, h = cam
    return minirt.Scene(meshes, lights, minirt.camera(eye, center, up, fovy, w, h), bg, amb, depth)


def load(defn):
    """(prepared HostScene, Oracle) of a definition, through write_sce and the product loader."""
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "scene.sce"
        minirt.write_sce(path, *defn)
        hs = rtamd.HostScene.load(path)
    hs.prepare()
    return hs, pyoracle.Oracle(hs.raw, hs)


_scenes, _frames, _far = {}, {}, {}


def _definition(key):
    kind = key[0]
    if kind == "fuzz":        # ("fuzz", transform name, seed, width, height)
        s, t = TRANSFORMS[key[1]]
        return transformed(key[2], s, t, key[3], key[4])
    if kind == "kat":         # ("kat", transform name, scene name)
        s, t = TRANSFORMS[key[1]]
        return transformed_kat(key[2], s, t)
    if kind == "variant":     # ("variant", variant name, seed)
        return variant(key[1], key[2])
    if kind == "scaled":      # ("scaled", s, seed): a scale outside the table
        return transformed(key[2], key[1], ZERO)
    raise KeyError(key)


def case(key):
    """(HostScene, Oracle) of a keyed scene, loaded once."""
    if key not in _scenes:
        _scenes[key] = load(_definition(key))
    return _scenes[key]


def fuzz_key(tname, seed, width=W, height=H):
    return ("fuzz", tname, seed, width, height)


def frame(key, spp, mode):
    """(image, Counts) of the oracle's render of a keyed scene's own camera, once per (key, spp, mode)."""
    k = (key, spp, mode)
    if k not in _frames:
        hs, orc = case(key)
        _frames[k] = orc.render(hs.render_params(0, 0, spp), mode)
    return _frames[k]


def rays_counted(cnt):
    return [int(cnt.primary_rays), int(cnt.shadow_rays), int(cnt.reflection_rays)]


def hit_fraction(tname):
    """(closest_hits, primary + reflection rays, shadow rays) of a transform, summed over SEEDS
    (reference mode, W x H, the seeds' own spp)."""
    hits = rays = shadow = 0
    for seed in SEEDS:
        _, cnt = frame(fuzz_key(tname, seed), spp_of(seed), REF)
        hits += int(cnt.closest_hits)
        rays += int(cnt.primary_rays) + int(cnt.reflection_rays)
        shadow += int(cnt.shadow_rays)
    return hits, rays, shadow


def check_not_vacuous(tname):
    """The conditions on the oracle's counts that make a comparison at this transform mean something."""
    hits, rays, shadow = hit_fraction(tname)
    if tname == ALL_REJECTED:
        assert hits == 0 and shadow == 0, (hits, shadow)
        return
    assert hits >= MIN_HIT_FRACTION * rays, (tname, hits, rays)
    if tname == PARTLY_REJECTED:
        h1, r1, _ = hit_fraction("identity")
        assert hits * r1 < h1 * rays, (hits, rays, h1, r1)


# ---- far-origin rays for the queries ----
def far_scene(name):
    """(HostScene, Oracle, vertex positions, vertex_idx, perm) of a generated scene (query_cases)."""
    return qc.scene(name, qc.SCENES[name].get("n_triangles", 0))


def scene_arrays(hs, orc):
    """(vertex positions, vertex_idx, perm) of a loaded scene, as query_cases.check_hits wants them."""
    soa = hs.soa_arrays()
    return soa["vertex_pos"], soa["vertex_idx"], orc.bvh()["perm"]


def far_rays(hs, dist_factor, n, seed, flavour="vertex", orc=None):
    """n rays whose origins lie dist_factor root-box diagonals from their targets:
    o = target + dist * u, d = target - o.
      "vertex": target a mesh vertex, u a random unit vector (ties and edges)
      "axis":   target uniform in the root box, u = +-e_k, d = -u (two exact zero components)
      "tmax":   target uniform in the root box, u random; a finite tmax drawn on both sides of
                the oracle's (ordered mode) hit distance: 0.5 t, the float below t, t, the float
                above t, 2 t in turn; half and twice the origin distance for the rays that miss"""
    rng = np.random.default_rng(seed)
    lo, hi = qc.root_box(hs)
    dist = dist_factor * float(np.sqrt(((hi - lo) ** 2).sum()))
    if flavour == "vertex":
        P = hs.soa_arrays()["vertex_pos"]
        target = P[rng.integers(0, len(P), n)]
    else:
        target = lo + rng.random((n, 3)) * (hi - lo)
    if flavour == "axis":
        u = np.zeros((n, 3))
        u[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
        d = -u
    else:
        u = rng.normal(size=(n, 3))
        u /= np.sqrt((u * u).sum(axis=1, keepdims=True))
        d = None
    o = target + dist * u
    rays = qc.make_rays(o, target - o if d is None else d)
    if flavour == "tmax":
        want = qc.oracle_hits(orc, rays, ORD)
        t = want["t"]
        pick = np.arange(n) % 5
        with np.errstate(invalid="ignore"):
            around = np.choose(pick, [0.5 * t, np.nextafter(t, 0.0), t, np.nextafter(t, np.inf), 2.0 * t])
        rays[:, 6] = np.where(want["hit"], around, np.where(pick < 2, 0.5 * dist, 2.0 * dist))
    return rays


def brute_force_t(hs, rays):
    """The smallest t the oracle's triangle test (or_intersect_triangle) accepts over ALL triangles
    of a loaded scene, per ray (inf: none), with no box in the way: what a traversal whose boxes
    are conservative must find.  Python loop over rays x triangles: scenes of a few hundred
    triangles only."""
    import ctypes as C

    fn = pyoracle.lib().or_intersect_triangle
    dp = C.POINTER(C.c_double)
    soa = hs.soa_arrays()
    P = np.ascontiguousarray(soa["vertex_pos"])
    corner = [[C.cast(P.ctypes.data + 24 * int(v), dp) for v in tri] for tri in soa["vertex_idx"]]
    o = np.ascontiguousarray(rays[:, 0:3])
    d = np.ascontiguousarray([qc.normalized(r) for r in rays[:, 3:6]])
    t, a, b, g = (C.c_double() for _ in range(4))
    out = np.full(len(rays), np.inf)
    for i in range(len(rays)):
        oi, di = C.cast(o.ctypes.data + 24 * i, dp), C.cast(d.ctypes.data + 24 * i, dp)
        best = np.inf
        for p0, p1, p2 in corner:
            if fn(p0, p1, p2, oi, di, C.byref(t), C.byref(a), C.byref(b), C.byref(g)) and t.value < best:
                best = t.value
        out[i] = best
    return out


def far_case(name, flavour, factor):
    """(rays, the oracle's ordered-mode hits with tmax = inf) of a far-ray set on a generated
    scene, 256 rays, once per key.  A ray counts as hit iff hit and t < rays[:, 6]."""
    key = (name, flavour, factor)
    if key not in _far:
        hs, orc, _, _, _ = far_scene(name)
        rays = far_rays(hs, factor, 256, 1 + FAR_FLAVOURS.index(flavour), flavour, orc)
        _far[key] = (rays, qc.oracle_hits(orc, rays, ORD))
    return _far[key]


def within_tmax(want, rays):
    """The oracle's hits cut at the rays' tmax: what rt_trace_closest returns."""
    keep = want["hit"] & (want["t"] < rays[:, 6])
    out = {k: v.copy() for k, v in want.items()}
    out["hit"] = keep
    out["t"][~keep] = np.inf
    out["tri"][~keep] = -1
    out["normal"][~keep] = 0.0
    out["point"][~keep] = 0.0
    return out
