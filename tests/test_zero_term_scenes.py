"""The zero-term scenes' own check (CPU): the oracle's reference mode and the pure-Python
restatement (tests/minirt.py) agree on every scene of tests/zero_term_scenes.py, and the scenes
hold what their GPU tests rely on."""
import numpy as np
import pytest

import minirt
import pyoracle
import rtamd
import zero_term_scenes as zts


@pytest.mark.parametrize("name", sorted(zts.scenes()))
def test_oracle_matches_python(tmp_path, name):
    hs = rtamd.HostScene.load(zts.write(tmp_path, name))
    hs.prepare()
    p = hs.render_params(0, 0, 1)
    img, cnt = pyoracle.Oracle(hs.raw, hs).render(p, pyoracle.MODE_REFERENCE)
    mini = zts.mini(name)
    ref = np.array(mini.render(1))
    assert img.shape == ref.shape
    assert np.abs(img - ref).max() <= 1e-12, np.abs(img - ref).max()
    assert [cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays] == \
        [mini.counts["primary"], mini.counts["shadow"], mini.counts["reflection"]]


def facing_away(mini):
    """(shadow rays, those with max(0, n.l) == 0) of the primary hits of a minirt scene."""
    c = mini.cam
    total = away = 0
    for y in range(c["h"]):
        for x in range(c["w"]):
            d = minirt.normalize(tuple(c["ll"][k] + x * c["xd"][k] + y * c["yd"][k] - c["eye"][k] for k in range(3)))
            h = mini.closest(c["eye"], d)
            if h is None:
                continue
            t, a, b, g, m, ti = h
            p = tuple(c["eye"][k] + t * d[k] for k in range(3))
            i0, i1, i2 = m.tris[ti]
            n = m.face_n[ti] if m.mode == "FLAT" else tuple(
                a * m.vert_n[i0][k] + b * m.vert_n[i1][k] + g * m.vert_n[i2][k] for k in range(3))
            for lpos, _ in mini.lights:
                total += 1
                away += not (minirt.dot(n, minirt.normalize(minirt.sub(lpos, p))) > 0.0)
    return total, away


def test_floor_scene_has_one_light_in_front_and_one_behind():
    total, away = facing_away(zts.mini("floor_two_lights"))
    assert total > 0 and 2 * away == total


def test_shininess_zero_changes_the_image():
    a = np.array(zts.mini("floor_two_lights").render(1))
    b = np.array(zts.mini("floor_shininess_zero").render(1))
    assert np.abs(a - b).max() > 0.05   # the light below adds ks * pow(0, 0) to every floor pixel


def test_terminator_scenes_have_both_signs():
    for name in ("phong_terminator", "one_light", "grazing", "many_lights"):
        total, away = facing_away(zts.mini(name))
        assert 0 < away < total, (name, total, away)


def test_phong_normals_are_not_unit():
    m = zts.mini("phong_terminator").meshes[1]
    i0, i1, i2 = m.tris[0]
    n = tuple((m.vert_n[i0][k] + m.vert_n[i1][k] + m.vert_n[i2][k]) / 3.0 for k in range(3))
    assert abs(minirt.dot(n, n) - 1.0) > 0.1
