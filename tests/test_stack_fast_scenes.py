"""The traversal-stack scenes' own check (CPU): the oracle alone pins the frames of
tests/stack_fast_scenes.py (ray counts, and the sum of the fp64 frame), so a change to a generator is
noticed, and shows that the scenes hold what tests/test_stack_fast_gpu.py relies on.  These are
conditions on the scenes, not measurements of the kernel."""
import numpy as np
import pytest

import minirt
import pyoracle
import rtamd
import stack_fast_scenes as sfs

# name: ([primary, shadow, reflection] rays, sum of the 64x48 fp64 frame), 1 spp, the oracle's ordered walk
PINS = {
    "deep": ([3072, 6180, 3081], 2246.47189749285),
    "flat": ([3072, 394, 0], 1365.836690614926),
    "occluder": ([3072, 4908, 733], 954.3654813738973),
    "fan": ([3072, 509, 325], 1365.3970685642705),
}


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    out = {}
    for name in sfs.NAMES:
        hs = rtamd.HostScene.load(sfs.write(name, tmp_path_factory.mktemp(name)))
        hs.prepare()
        out[name] = (hs, pyoracle.Oracle(hs.raw, hs))
    return out


def counts(c):
    return [c.primary_rays, c.shadow_rays, c.reflection_rays]


@pytest.mark.parametrize("name", sfs.NAMES)
def test_frame_is_pinned(scenes, name):
    hs, orc = scenes[name]
    p = hs.render_params(0, 0, 1)
    assert (p.camera.width, p.camera.height) == (sfs.W, sfs.H)
    img, cnt = orc.render(p, pyoracle.MODE_ORDERED)
    print(name, counts(cnt), repr(float(img.sum())))
    rays, total = PINS[name]
    assert counts(cnt) == rays
    assert abs(float(img.sum()) - total) <= 1e-9 * total


@pytest.mark.parametrize("name", sfs.NAMES)
def test_oracle_modes_agree(scenes, name):
    # no ray of these frames sits on a tie or on a box face: the oracle's unordered reference walk and
    # its ordered, culled one (the kernel's algorithm) find the same hits.  The deep scene's reference
    # walk tests every triangle for every ray: every fifth pixel of every fifth row there.
    hs, orc = scenes[name]
    p = hs.render_params(0, 0, 1)
    step = 5 if name == "deep" else 1
    xy = np.stack(np.meshgrid(np.arange(0, sfs.W, step), np.arange(0, sfs.H, step)), -1).reshape(-1, 2).astype(np.int32)
    a, ca = orc.render_pixels(p, xy, pyoracle.MODE_REFERENCE)
    b, cb = orc.render_pixels(p, xy, pyoracle.MODE_ORDERED)
    assert np.abs(a - b).max() <= 1e-12
    assert counts(ca) == counts(cb)


def test_small_scenes_match_the_python_renderer(tmp_path):
    for name in ("flat", "fan"):
        meshes, lights, cam, depth = sfs.scene(name)
        eye, center, up, fovy = cam[:4]
        size = (16, 12)
        mini = minirt.Scene(meshes, lights, minirt.camera(eye, center, up, fovy, *size), sfs.BG, sfs.AMB, depth)
        path = tmp_path / f"{name}_small.sce"
        minirt.write_sce(path, meshes, lights, cam[:4] + size, sfs.BG, sfs.AMB, depth)
        hs = rtamd.HostScene.load(path)
        hs.prepare()
        img, cnt = pyoracle.Oracle(hs.raw, hs).render(hs.render_params(0, 0, 1), pyoracle.MODE_REFERENCE)
        ref = np.array(mini.render(1))
        assert np.abs(img - ref).max() <= 1e-12
        assert counts(cnt) == [mini.counts["primary"], mini.counts["shadow"], mini.counts["reflection"]]


def test_deep_scene_every_box_holds_every_ray(scenes):
    """Every triangle's bounding box spans the view cone's cross-section at its depth, so any box over
    any subset of them contains every primary ray between its nearest and its farthest triangle: a ray
    meets all children of every node above its hit."""
    hs, _ = scenes["deep"]
    tris = np.array(sfs.deep_triangles())            # [n, 3, 3]
    d = -tris[:, :2, 2].mean(1)                      # the two corner vertices stand at z = -d
    half_h = np.tan(np.radians(sfs.DEEP_FOVY / 2))
    half_w = half_h * sfs.W / sfs.H
    lo, hi = tris.min(1), tris.max(1)
    assert (lo[:, 0] <= -half_w * d).all() and (hi[:, 0] >= half_w * d).all()
    assert (lo[:, 1] <= -half_h * d).all() and (hi[:, 1] >= half_h * d).all()
    assert len(tris) == sfs.DEEP_N >= 4 ** 8          # eight 4-wide levels even with one triangle per leaf
    assert hs.bvh_depth >= 15


def test_flat_scene_is_two_levels(scenes):
    hs, _ = scenes["flat"]
    assert len(sfs.flat_triangles()) == 12 and hs.bvh_depth <= 4


def test_occluder_scene_has_lit_shadowed_and_mixed_tiles(scenes):
    """Per 8x8 tile (one wave's pixels) of the primary hits on the floor: how many see a light.  Tiles
    that see none, tiles where every pixel sees one, and tiles with both occur; mirror tents send
    reflection rays from the same tiles."""
    hs, orc = scenes["occluder"]
    p = hs.render_params(0, 0, 1)
    assert p.n_lights == 2
    eye, center, up, fovy = sfs.OCC_CAM[:4]
    c = minirt.camera(eye, center, up, fovy, sfs.W, sfs.H)
    tiles = {}
    for y in range(sfs.H):
        for x in range(sfs.W):
            d = minirt.normalize(tuple(c["ll"][k] + x * c["xd"][k] + y * c["yd"][k] - c["eye"][k] for k in range(3)))
            h = orc.closest_hit(eye, d)
            if h is None:
                continue
            lit = 0
            for lpos, _ in sfs.OCC_LIGHTS:
                to_l = minirt.sub(lpos, tuple(h["point"]))
                l = minirt.normalize(to_l)
                s = orc.closest_hit(tuple(h["point"][k] + 1e-4 * l[k] for k in range(3)), l)
                lit += not (s is not None and s["t"] < np.sqrt(minirt.dot(to_l, to_l)))
            t = tiles.setdefault((x // 8, y // 8), [0, 0])
            t[lit > 0] += 1
    dark = sum(1 for a, b in tiles.values() if b == 0)
    bright = sum(1 for a, b in tiles.values() if a == 0)
    mixed = sum(1 for a, b in tiles.values() if a > 0 and b > 0)
    print(f"tiles: no light {dark}, every pixel lit {bright}, both {mixed}")
    assert dark >= 4 and bright >= 4 and mixed >= 4
    _, cnt = orc.render(p, pyoracle.MODE_ORDERED)
    assert cnt.reflection_rays > 0 and cnt.shadow_rays > 0


def test_fan_scene_rays_meet_zero_to_four_boxes():
    boxes = sfs.fan_boxes()
    eye, center, up, fovy = sfs.FAN_CAM[:4]
    c = minirt.camera(eye, center, up, fovy, sfs.W, sfs.H)
    seen = {}
    for y in range(sfs.H):
        for x in range(sfs.W):
            d = minirt.normalize(tuple(c["ll"][k] + x * c["xd"][k] + y * c["yd"][k] - c["eye"][k] for k in range(3)))
            n = sum(1 for lo, hi in boxes if pyoracle.intersect_aabb(eye, d, lo, hi))
            seen[n] = seen.get(n, 0) + 1
    print("pixels by boxes met:", dict(sorted(seen.items())))
    assert set(seen) == {0, 1, 2, 3, 4}
    assert min(seen.values()) >= 32
