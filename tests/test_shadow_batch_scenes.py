"""The shadow-batch scenes' own check (CPU): the oracle's reference mode and the pure-Python
restatement (tests/minirt.py) agree on every scene of tests/shadow_batch_scenes.py, and the scenes
hold what their GPU tests rely on.  Small images: the scenes are what is checked here, and minirt
is slow."""
import numpy as np
import pytest

import minirt
import pyoracle
import rtamd
import shadow_batch_scenes as sbs

SIZE = (16, 12)


@pytest.mark.parametrize("name", sorted(sbs.scenes()))
def test_oracle_matches_python(tmp_path, name):
    size = (8, 8) if name == "floor_fill" else SIZE
    hs = rtamd.HostScene.load(sbs.write(tmp_path, name, size))
    hs.prepare()
    p = hs.render_params(0, 0, 1)
    img, cnt = pyoracle.Oracle(hs.raw, hs).render(p, pyoracle.MODE_REFERENCE)
    mini = sbs.mini(name, size)
    ref = np.array(mini.render(1))
    assert img.shape == ref.shape
    assert np.abs(img - ref).max() <= 1e-12, np.abs(img - ref).max()
    assert [cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays] == \
        [mini.counts["primary"], mini.counts["shadow"], mini.counts["reflection"]]


def light_classes(mini):
    """Primary hits of a minirt scene and, per light, the hit points that see it, that are shadowed
    from it, and that face away from it (max(0, n.l) == 0: the zero-term rays)."""
    c = mini.cam
    hits = 0
    lit, dark, away = ([0] * len(mini.lights) for _ in range(3))
    for y in range(c["h"]):
        for x in range(c["w"]):
            d = minirt.normalize(tuple(c["ll"][k] + x * c["xd"][k] + y * c["yd"][k] - c["eye"][k] for k in range(3)))
            h = mini.closest(c["eye"], d)
            if h is None:
                continue
            hits += 1
            t, a, b, g, m, ti = h
            p = tuple(c["eye"][k] + t * d[k] for k in range(3))
            n = m.face_n[ti]
            for j, (lpos, _) in enumerate(mini.lights):
                to_l = minirt.sub(lpos, p)
                l = minirt.normalize(to_l)
                if not (minirt.dot(n, l) > 0.0):
                    away[j] += 1
                    continue
                s = mini.closest(tuple(p[k] + 1e-4 * l[k] for k in range(3)), minirt.normalize(l))
                if s is not None and 0.0 < s[0] < minirt.dot(to_l, to_l) ** 0.5:
                    dark[j] += 1
                else:
                    lit[j] += 1
    return hits, lit, dark, away


@pytest.mark.parametrize("n", sbs.LIGHT_COUNTS)
def test_lights_are_seen_shadowed_and_behind(n):
    mini = sbs.mini(f"lights{n}_depth0", SIZE)
    hits, lit, dark, away = light_classes(mini)
    assert 2 * hits > SIZE[0] * SIZE[1]          # most primary rays hit a shadowable surface
    below = [pos[1] < 0.0 for pos, _ in mini.lights]
    # every light above the floor is seen from some hit points and not from others; the floor hides
    # the ones below it from every hit point that faces them
    assert all(v > 0 for v, u in zip(lit, below) if not u)
    assert all(v == 0 for v, u in zip(lit, below) if u)
    assert all(d + a > 0 for d, a in zip(dark, away))
    assert sum(dark) > 0 and sum(away) > 0
    if n > 1:
        assert away[1] >= hits // 2              # the second light is below the floor


def test_floor_fills_the_view():
    mini = sbs.mini("floor_fill", (16, 16))
    hits, lit, dark, away = light_classes(mini)
    assert hits == 16 * 16
    assert lit == [hits, hits] and sum(dark) + sum(away) == 0
