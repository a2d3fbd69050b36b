"""Scenes for rt_scene_update_positions, rt_scene_set_triangle_order and rt_normals_host (DESIGN.md
§26), shared by tests/test_positions_host.py, tests/test_positions_abi.py (CPU) and
tests/test_positions_gpu.py (GPU).  The moved fuzz, office and cornell scenes are
tests/update_cases.py's; two scenes are added here, minirt meshes written with minirt.write_sce and
read back by the product loader, 32 x 24:

  fan         a floor and one PHONG mesh of FAN_N = 100 triangles that share one apex (a valence
              above a wave's 64 lanes: the long CSR walk) plus one vertex no triangle references,
              which holds the largest |coordinate| of the scene and is negative: it decides delta
              but not the root box.  B: every vertex jittered, that vertex moved further out.
  degenerate  a floor and one PHONG mesh with a triangle that names one vertex twice, a zero-area
              triangle of three collinear distinct vertices, a triangle so thin that the weight of
              its obtuse corner is non-zero with |w| <= 1e-12 (that corner is skipped, not added as
              zero), and ordinary triangles that share vertices with them.  B: that mesh scaled by
              1/2 (exact: collinear stays collinear, the thin weight stays under the threshold), the
              floor jittered.

case(key) hands out a scene of its own each time, which the caller may move."""
import ctypes as C
import functools
import math

import numpy as np

import fuzz_scenes
import minirt
import rtamd
import scale_scenes as ss
import update_cases as uc

W, H = uc.W, uc.H
FAN_N = 100
MADE = ("fan", "degenerate")
EPS = 1e-12   # compute_normals' threshold on a corner weight

_MAT_A = ((0.1, 0.1, 0.1), (0.7, 0.6, 0.5), (0.3, 0.3, 0.3), 20.0, 0.0, 1)
_MAT_B = ((0.05, 0.1, 0.1), (0.3, 0.6, 0.8), (0.5, 0.5, 0.5), 64.0, 0.3, 1)
_FLOOR = ([(-3.0, -1.0, -3.0), (3.1, -1.0, -3.0), (3.0, -1.0, 3.2), (-3.1, -1.0, 3.0)], [(0, 2, 1), (0, 3, 2)])
_LIGHTS = [((2.0, 4.0, 3.0), (0.9, 0.9, 0.8)), ((-3.0, 2.5, 1.0), (0.3, 0.3, 0.4))]
FAN_LONER = (-50.0, 0.25, 0.5)
# the odd mesh of `degenerate`: vertices and triangles
_ODD_V = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.0),                 # 0-2 collinear
          (-1.0, 0.5, 0.0), (1.0, 0.5, 0.0), (0.0, 0.5 + 1e-7, 0.0),         # 3-5 thin: the corner at 5 is ~pi
          (0.0, 1.0, 0.0), (1.0, 1.5, 0.2),                                  # 6-7: (6, 6, 7)
          (-1.0, -0.5, 0.5), (1.0, -0.5, 0.5), (0.0, 1.2, -0.5)]             # 8-10 ordinary
ODD_TWICE, ODD_COLLINEAR, ODD_THIN = (6, 6, 7), (0, 1, 2), (5, 3, 4)
_ODD_T = [(8, 9, 10), ODD_TWICE, (8, 10, 3), ODD_COLLINEAR, (9, 4, 10), ODD_THIN, (3, 10, 6), (0, 8, 5), (7, 4, 2)]


@functools.lru_cache(maxsize=None)
def definition(name):
    floor = minirt.Mesh(_FLOOR[0], _FLOOR[1], "FLAT", _MAT_A)
    if name == "fan":
        ring = [(1.5 * math.cos(2.0 * math.pi * i / FAN_N), 0.3 * math.sin(14.0 * math.pi * i / FAN_N),
                 1.5 * math.sin(2.0 * math.pi * i / FAN_N)) for i in range(FAN_N)]
        verts = [(0.0, 1.0, 0.0)] + ring + [FAN_LONER]
        tris = [(0, 1 + (i + 1) % FAN_N, 1 + i) for i in range(FAN_N)]
        cam = ((0.5, 3.0, 4.0), (0.0, 0.2, 0.0), (0.0, 1.0, 0.0), 50.0, W, H)
        return [floor, minirt.Mesh(verts, tris, "PHONG", _MAT_B)], _LIGHTS, cam, (0.1, 0.1, 0.2), (0.2, 0.2, 0.2), 1
    if name == "degenerate":
        cam = ((0.3, 0.8, 4.0), (0.3, 0.3, 0.0), (0.0, 1.0, 0.0), 50.0, W, H)
        return [floor, minirt.Mesh(_ODD_V, _ODD_T, "PHONG", _MAT_B)], _LIGHTS, cam, (0.1, 0.1, 0.2), (0.2, 0.2, 0.2), 1
    raise KeyError(name)


def load(name):
    """A new prepared HostScene of a made scene."""
    return ss.load(definition(name))[0]


def pos_b(hs, name):
    """B's positions in global vertex order."""
    soa = hs.soa_arrays()
    P, mid = soa["vertex_pos"].copy(), soa["vertex_mesh_id"]
    rng = np.random.default_rng(7)
    if name == "fan":
        P += 0.05 * rng.uniform(-1.0, 1.0, size=P.shape)
        P[unreferenced(hs)] = (-60.0, 0.5, 0.25)
    else:
        P[mid == 1] *= 0.5
        P[mid == 0] += 0.05 * rng.uniform(-1.0, 1.0, size=(int((mid == 0).sum()), 3))
    return P


def unreferenced(hs):
    """Global ids of the vertices no triangle references."""
    soa = hs.soa_arrays()
    used = np.zeros(len(soa["vertex_pos"]), dtype=bool)
    used[soa["vertex_idx"].reshape(-1)] = True
    return np.flatnonzero(~used)


KEYS = tuple(("fuzz", s) for s in uc.KEPT) + tuple(("gen", n) for n in uc.GENERATED) + tuple(("made", n) for n in MADE)


def case(key):
    """(a new prepared HostScene of A, posB) of ("fuzz", seed), ("gen", name) or ("made", name)."""
    kind, which = key
    if kind == "fuzz":
        return ss.load(fuzz_scenes.scene(which, W, H))[0], uc.pos_b(which)
    if kind == "gen":
        hs = uc.generated(which)
        return hs, uc.generated_pos_b(hs)
    hs = load(which)
    return hs, pos_b(hs, which)


def frame_size(key):
    """(width, height) of a case's test frames: the generated scenes' own cameras are large."""
    return (64, 36) if key[0] == "gen" else (0, 0)


def corner_weights(P, tri):
    """The three corner weights of triangle `tri` of positions P, as compute_normals forms them."""
    p0, p1, p2 = (tuple(float(x) for x in P[i]) for i in tri)
    a, b, c = minirt.sub(p1, p0), minirt.sub(p2, p1), minirt.sub(p0, p2)
    la, lb, lc = (math.sqrt(minirt.dot(v, v)) for v in (a, b, c))
    neg = lambda v: (-v[0], -v[1], -v[2])  # noqa: E731
    return (la * lc + minirt.dot(a, neg(c)), lb * la + minirt.dot(b, neg(a)), lc * lb + minirt.dot(c, neg(b)))


def normals_host(hs, pos):
    """rt_normals_host on the scene's leaf-order vertex ids and slot_triangles():
    (vertex_normals [nv, 3], face_normals [nt, 3] in leaf order)."""
    soa = hs.soa_arrays()
    vidx = np.ascontiguousarray(soa["vertex_idx"], dtype=np.int32)
    order = hs.slot_triangles()
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    vn, fn = np.full((len(pos), 3), np.nan), np.full((len(vidx), 3), np.nan)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    rc = rtamd.hip_lib().rt_normals_host(vidx.ctypes.data_as(ip), order.ctypes.data_as(ip), len(pos), len(vidx),
                                         pos.ctypes.data_as(dp), vn.ctypes.data_as(dp), fn.ctypes.data_as(dp))
    assert rc == 0, rtamd.hip_lib().rt_last_error()
    return vn, fn


def bits(a):
    """The array's bytes as uint64, for == on doubles that tells -0.0 from +0.0 and NaN payloads apart."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
