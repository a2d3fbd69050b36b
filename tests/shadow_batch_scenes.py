"""Scenes for the shadow-batch tests: a bounce's shadow rays for 1 .. 64 lights, with
lights that are visible from some hit points, occluded from others and behind the surface (zero
term) for others still.  Written as .sce/.obj and loaded through the product loader, like
tests/zero_term_scenes.py; tests/test_shadow_batch_scenes.py pins them (oracle against
tests/minirt.py)."""
import math

import minirt
from zero_term_scenes import MIRROR, SHINY, octahedron

LIGHT_COUNTS = (1, 2, 3, 32, 33, 64)

# a floor y = 0 (face normal +y) wider than the view, an octahedron standing over it
WIDE_V = [(-9.0, 0.0, 9.0), (9.0, 0.0, 9.0), (9.0, 0.0, -9.0), (-9.0, 0.0, -9.0)]
FLOOR_T = [(0, 1, 2), (0, 2, 3)]
CAM = ((0.113, 3.521, 4.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 40.0, 64, 48)
# straight down on one of the floor's two triangles (the view stays clear of their shared edge
# x = -z, where a ray can slip between them): every pixel hits
CAM_DOWN = ((3.07, 5.0, 2.55), (3.0, 0.0, 2.5), (0.0, 0.0, -1.0), 40.0, 64, 64)


def ring_lights(n):
    """n lights on a golden-angle spiral around the octahedron: most above the floor at several
    heights (the octahedron shadows part of the floor from each, and faces half of its sides away
    from each), every fifth one (the second first) below the floor, where the floor's term is zero and
    the floor hides it from the octahedron's lower faces."""
    out = []
    for i in range(n):
        a = 2.399963 * i + 0.4
        r = 1.6 + 0.45 * (i % 5)
        y = 0.6 + 0.7 * (i % 4)
        if i % 5 == 1:
            y = -(1.2 + 0.05 * i)
        s = 1.3 / n
        col = (s * (0.8 + 0.02 * (i % 7)), s * (0.75 + 0.03 * (i % 5)), s * (0.7 + 0.04 * (i % 3)))
        out.append(((r * math.cos(a), y, r * math.sin(a)), col))
    return out


def scenes():
    """name -> (meshes, lights, cam_def, background, ambience, max_depth)."""
    out = {}
    bg, amb = (0.05, 0.1, 0.2), (0.2, 0.2, 0.2)
    ov, ot = octahedron((0.0, 1.1, 0.0), 1.0)
    for n in LIGHT_COUNTS:
        for depth in (0, 3):
            meshes = [minirt.Mesh(WIDE_V, FLOOR_T, "FLAT", MIRROR), minirt.Mesh(ov, ot, "FLAT", SHINY)]
            out[f"lights{n}_depth{depth}"] = (meshes, ring_lights(n), CAM, bg, amb, depth)
    # the floor alone, seen from straight above: every pixel hits, every lane of every wave is in step
    out["floor_fill"] = ([minirt.Mesh(WIDE_V, FLOOR_T, "FLAT", SHINY)],
                         [((3.8, 4.0, 3.0), (0.5, 0.5, 0.5)), ((1.9, 3.0, 1.8), (0.4, 0.4, 0.3))], CAM_DOWN, bg, amb, 0)
    return out


def _scene(name, size):
    meshes, lights, cam_def, bg, amb, depth = scenes()[name]
    if size is not None:
        cam_def = cam_def[:4] + tuple(size)
    return meshes, lights, cam_def, bg, amb, depth


def write(tmpdir, name, size=None):
    meshes, lights, cam_def, bg, amb, depth = _scene(name, size)
    path = tmpdir / f"{name}.sce"
    minirt.write_sce(path, meshes, lights, cam_def, bg, amb, depth)
    return path


def mini(name, size=None):
    meshes, lights, cam_def, bg, amb, depth = _scene(name, size)
    eye, center, up, fovy, w, h = cam_def
    return minirt.Scene(meshes, lights, minirt.camera(eye, center, up, fovy, w, h), bg, amb, depth)
