"""Scenes, option sets and the numpy reference of the re-clipping update (rt_scene_update_vertices_ex
with RT_UPDATE_RECLIP), shared by tests/test_reclip_host.py, tests/test_reclip_abi.py
(CPU) and tests/test_reclip_gpu.py (GPU).

The scenes are tests/update_cases.py's: fuzz seeds 0, 1, 2 and 6 at 32 x 24 moved by 0.2 of the
diagonal, cornell and office with their odd meshes translated.  Two option sets: the defaults, and
spatial splits wherever they pay (sbvh_alpha 0, sbvh_budget 1.5; single-record leaves on the fuzz
scenes).  Seeds 1 and 2 hold cut records under both and seed 0 under "split" (at the defaults its
119 triangles have 119 records); seed 6 holds none under either: the no-table cases.

Everything computed here is cached per key and shared; callers must not modify it."""
import functools

import numpy as np

import rtamd
import update_cases as uc

CUT_SEEDS = (0, 1, 2)
PLAIN_SEED = 6
OPTION_SETS = {"default": {}, "split": {"sbvh_alpha": 0.0, "sbvh_budget": 1.5}}
# records at (default, split) options, by rtamd.tree_report on the CPU
RECORDS = {0: (119, 125), 1: (62, 63), 2: (56, 56), 6: (21, 21), "cornell": (3730, 6629), "office": (76009, 149175)}
TRIANGLES = {0: 119, 1: 59, 2: 55, 6: 21, "cornell": 2906, "office": 59670}
# (fuzz seed, option set) with cut records, and without
CUT_FUZZ = tuple((s, o) for s in CUT_SEEDS for o in sorted(OPTION_SETS) if RECORDS[s][o == "split"] > TRIANGLES[s])
UNCUT_FUZZ = tuple((s, o) for s in CUT_SEEDS + (PLAIN_SEED,) for o in sorted(OPTION_SETS)
                   if RECORDS[s][o == "split"] == TRIANGLES[s])


def options(scene, oset):
    """Upload options of option set `oset` for a fuzz seed (int) or a generated scene (name)."""
    o = dict(OPTION_SETS[oset])
    if oset == "split" and isinstance(scene, int):
        o["sbvh_leaf_max"] = 1
    return o


@functools.lru_cache(maxsize=None)
def host_a(scene):
    """The shared, unmoved HostScene of a fuzz seed or a generated scene."""
    return uc.fuzz_a(scene)[0] if isinstance(scene, int) else uc.generated(scene)


@functools.lru_cache(maxsize=None)
def regions(scene, oset):
    """(clip [records, 6], slot [records]) of rtamd.clip_regions."""
    return rtamd.clip_regions(host_a(scene), **options(scene, oset))


def assert_cut(scene, oset):
    """Non-vacuity of a test that claims to exercise re-clipping: duplicated references and at least
    one finite clip plane.  Returns (clip, slot)."""
    clip, slot = regions(scene, oset)
    assert len(clip) > TRIANGLES[scene], (scene, oset)
    assert np.isfinite(clip).any(), (scene, oset)
    return clip, slot


def moved(scene):
    """A new HostScene moved to B that the caller may move again."""
    if isinstance(scene, int):
        return uc.updated(scene)
    hs = uc.generated(scene)
    hs.update_vertices(uc.generated_pos_b(hs))
    return hs


# ---- numpy fp64 reference: Sutherland-Hodgman clip of a triangle to an axis-aligned region ----
def _clip_plane(poly, k, pos, upper):
    inside = (lambda p: p[k] <= pos) if upper else (lambda p: p[k] >= pos)
    out = []
    for i, a in enumerate(poly):
        b = poly[(i + 1) % len(poly)]
        if inside(a):
            out.append(a)
        if inside(a) != inside(b):
            t = (pos - a[k]) / (b[k] - a[k])
            p = a + t * (b - a)
            p[k] = pos
            out.append(p)
    return out


def sh_clip(tri, clip):
    """The polygon (list of float64 [3] points, possibly empty) of triangle tri [3, 3] inside region
    clip [6] (lo xyz, hi xyz; closed half-spaces), one finite plane after the other."""
    poly = [np.array(v, dtype=np.float64) for v in tri]
    for k in range(3):
        for pos, upper in ((clip[k], False), (clip[3 + k], True)):
            if np.isfinite(pos) and poly:
                poly = _clip_plane(poly, k, float(pos), upper)
    return poly


def candidates(tri, clip):
    """The points the device's edge walk looks at: the three vertices and, per finite plane, the
    crossing points of the edges (p = a + t (b - a), t = (pos - a[k]) / (b[k] - a[k]), p[k] = pos)."""
    pts = [np.array(v, dtype=np.float64) for v in tri]
    for k in range(3):
        for pos in (clip[k], clip[3 + k]):
            if not np.isfinite(pos):
                continue
            for e in range(3):
                a, b = pts[e], pts[(e + 1) % 3]
                if (a[k] < pos and b[k] > pos) or (a[k] > pos and b[k] < pos):
                    t = (pos - a[k]) / (b[k] - a[k])
                    p = a + t * (b - a)
                    p[k] = pos
                    pts.append(p)
    return pts


def in_region(p, clip):
    return bool(np.all(p >= clip[:3]) and np.all(p <= clip[3:]))
