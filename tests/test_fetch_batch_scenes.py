"""The record-fetch scenes' own check (CPU): the oracle alone shows that the scenes of
tests/fetch_batch_scenes.py hold what tests/test_fetch_batch_gpu.py relies on.  These are conditions
on the scenes, not measurements of the kernel."""
import math

import numpy as np
import pytest

import fetch_batch_scenes as fbs
import minirt
import pyoracle
import rtamd


def primary_dirs(mini):
    c = mini.cam
    for y in range(c["h"]):
        for x in range(c["w"]):
            yield x, y, minirt.normalize(tuple(c["ll"][k] + x * c["xd"][k] + y * c["yd"][k] - c["eye"][k] for k in range(3)))


@pytest.fixture(scope="module")
def leaf(tmp_path_factory):
    hs = rtamd.HostScene.load(fbs.write_leaf(tmp_path_factory.mktemp("leaf")))
    hs.prepare()
    return hs, pyoracle.Oracle(hs.raw, hs)


def test_leaf_scene_oracle_matches_python(tmp_path):
    size = (16, 12)
    hs = rtamd.HostScene.load(fbs.write_leaf(tmp_path, size))
    hs.prepare()
    img, cnt = pyoracle.Oracle(hs.raw, hs).render(hs.render_params(0, 0, 1), pyoracle.MODE_REFERENCE)
    mini = fbs.mini_leaf(size)
    ref = np.array(mini.render(1))
    assert np.abs(img - ref).max() <= 1e-12, np.abs(img - ref).max()
    assert [cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays] == \
        [mini.counts["primary"], mini.counts["shadow"], mini.counts["reflection"]]
    assert cnt.shadow_rays > 0 and cnt.reflection_rays > 0


def test_leaf_scene_has_leaves_of_one_to_five_and_more_records(leaf):
    _, orc = leaf
    sizes = set(int(n) for n in orc.bvh()["tri_count"] if n > 0)
    print("leaf sizes of the reference tree:", sorted(sizes))
    assert {1, 2, 3, 4, 5} <= sizes and max(sizes) > 5


def test_leaf_scene_stands_far_from_the_origin_in_y_and_z():
    clusters, shelves, wall = fbs.leaf_triangles()
    v = np.array([p for t in clusters + shelves + wall for p in t])
    assert np.abs(v[:, 0]).max() <= 4.0 and v[:, 1].min() >= 28.0 and v[:, 2].max() <= -60.0


def test_leaf_scene_skips_and_takes_the_degenerate_branch(leaf):
    """The reference traversal (oracle/rt_oracle.c bvh_ref: every triangle of every leaf whose box, and
    whose ancestors' boxes, the ray meets) of the primary rays, restated on the exported tree: the
    triangle tests with |S| < 1e-10 (branch skipped) and the others (taken), in all and per 8x8 tile."""
    hs, orc = leaf
    mini = fbs.mini_leaf()
    b = orc.bvh()
    # triangles in leaf order: leaf slot -> vertices (perm maps the slot to the input triangle)
    tris = [t for m in mini.meshes for t in ([m.verts[i] for i in tri] for tri in m.tris)]
    perm = b["perm"]
    eye = mini.cam["eye"]
    skipped = taken = 0
    tiles = {}

    def walk(node, d, out):
        if not pyoracle.intersect_aabb(eye, d, b["bb_min"][node], b["bb_max"][node]):
            return
        n = int(b["tri_count"][node])
        if n > 0:
            out.extend(range(int(b["first_tri"][node]), int(b["first_tri"][node]) + n))
            return
        l = int(b["left_child"][node])
        walk(l, d, out)
        walk(l + 1, d, out)

    for x, y, d in primary_dirs(mini):
        slots = []
        walk(0, d, slots)
        c3 = (-d[0], -d[1], -d[2])
        for s in slots:
            p0, p1, p2 = tris[perm[s]]
            S = minirt.det3(minirt.sub(p0, p2), minirt.sub(p1, p2), c3)
            skip = abs(S) < 1e-10
            skipped += skip
            taken += not skip
            t = tiles.setdefault((x // 8, y // 8), [0, 0])
            t[skip] += 1
    # the restatement counts what the oracle counts
    p = hs.render_params(0, 0, 1)
    p.n_lights = 0
    p.max_depth = 0
    _, cnt = orc.render(p, pyoracle.MODE_REFERENCE)
    assert cnt.primary_rays == fbs.W * fbs.H and cnt.shadow_rays == cnt.reflection_rays == 0
    assert cnt.tri_tests == skipped + taken
    mixed = sum(1 for t in tiles.values() if t[0] > 0 and t[1] > 0)
    print(f"triangle tests {skipped + taken}: branch skipped {skipped}, taken {taken}; tiles with both {mixed} of 48")
    assert skipped >= 0.01 * (skipped + taken)
    assert taken >= 0.50 * (skipped + taken)
    assert mixed >= 24   # lanes of one wave skip and take together
    # the middle pixel row's rays are horizontal: the shelves are edge-on to them
    mid = [d for x, y, d in primary_dirs(mini) if y == fbs.H // 2]
    assert all(abs(d[1]) < 1e-12 for d in mid)


@pytest.mark.parametrize("name", ["leaf", "material"])
def test_oracle_modes_agree(tmp_path, name):
    # no ray of these frames sits on a tie or on a box face: the oracle's unordered reference walk
    # and its ordered, culled one (the kernel's algorithm) find the same hits
    hs = rtamd.HostScene.load((fbs.write_leaf if name == "leaf" else fbs.write_material)(tmp_path))
    hs.prepare()
    orc = pyoracle.Oracle(hs.raw, hs)
    for spp in (1, 2):
        p = hs.render_params(0, 0, spp)
        a, ca = orc.render(p, pyoracle.MODE_REFERENCE)
        b, cb = orc.render(p, pyoracle.MODE_ORDERED)
        assert np.abs(a - b).max() <= 1e-12
        assert [ca.primary_rays, ca.shadow_rays, ca.reflection_rays] == [cb.primary_rays, cb.shadow_rays, cb.reflection_rays]


def sphere_t(o, d):
    c, r, _ = fbs.SPHERE
    oc = minirt.sub(o, c)
    a, bq, cq = minirt.dot(d, d), 2.0 * minirt.dot(d, oc), minirt.dot(oc, oc) - r * r
    disc = bq * bq - 4.0 * a * cq
    if disc < 0.0:
        return math.inf
    ts = [t for t in ((-bq - math.sqrt(disc)) / (2.0 * a), (-bq + math.sqrt(disc)) / (2.0 * a)) if t > 1e-5]
    return min(ts, default=math.inf)


def test_material_scene_mixes_the_kinds_within_tiles(tmp_path):
    hs = rtamd.HostScene.load(fbs.write_material(tmp_path))
    hs.prepare()
    assert hs.raw.contents.n_spheres == 1 and hs.raw.contents.n_planes == 0
    p = hs.render_params(0, 0, 1)
    assert p.n_lights == 2 and p.max_depth == 3 and (p.camera.width, p.camera.height) == (fbs.W, fbs.H)
    orc = pyoracle.Oracle(hs.raw, hs)
    names = list(fbs.KINDS)
    first = np.cumsum([0] + [len(t) for _, t, _ in fbs.tent_meshes().values()])   # mesh -> first triangle id
    eye, center, up, fovy = fbs.MAT_CAM[:4]
    cam = {"cam": minirt.camera(eye, center, up, fovy, fbs.W, fbs.H)}
    scene = type("S", (), cam)
    seen = {}
    tiles = {}
    for x, y, d in primary_dirs(scene):
        h = orc.closest_hit(eye, d)
        ts = sphere_t(eye, d)
        if h is None and ts == math.inf:
            continue
        if h is None or h["tri"] < 0 or ts <= h["t"]:   # (the oracle's closest hit may be the sphere itself)
            kind = "sphere"
        else:
            kind = names[int(np.searchsorted(first, h["tri"], side="right")) - 1]
        seen[kind] = seen.get(kind, 0) + 1
        tiles.setdefault((x // 8, y // 8), set()).add(kind)
    print("pixels per kind:", seen)
    assert set(seen) == set(names) | {"sphere"}
    assert min(seen.values()) >= 32
    rich = sum(1 for k in tiles.values() if len(k) >= 3)
    print("tiles with three or more kinds:", rich)
    assert rich >= 4
    # the kinds cover both draw modes, both texture states, both shadow states and both mirror states
    for pick in (lambda k: k[0], lambda k: k[1], lambda k: k[2][5], lambda k: k[2][4] > 0.0):
        assert len({pick(k) for k in fbs.KINDS.values()}) == 2
    # the full render sends shadow and reflection rays (depth 3), also from the sphere
    _, cnt = orc.render(p, pyoracle.MODE_REFERENCE)
    assert cnt.shadow_rays > 0 and cnt.reflection_rays > 0
