"""Scenes for the zero-term shadow-ray tests: lights that face away from the
surface they would light, so that their Lambert and Phong terms are exactly 0 and the kernel does
not trace their shadow rays.  Written as .sce/.obj and loaded through the product loader, like
tests/kat_scenes.py; tests/test_zero_term_scenes.py pins them (oracle against tests/minirt.py)."""
import minirt

SHINY = ((0.1, 0.1, 0.1), (0.7, 0.6, 0.5), (0.3, 0.3, 0.3), 20.0, 0.0, 1)
DULL = ((0.1, 0.1, 0.1), (0.7, 0.6, 0.5), (0.3, 0.3, 0.3), 0.0, 0.0, 1)      # shininess 0: pow(0, 0) = 1
MIRROR = ((0.05, 0.05, 0.05), (0.2, 0.3, 0.2), (0.5, 0.5, 0.5), 40.0, 0.6, 1)

# floor y = 0, face normal +y
FLOOR_V = [(-3.0, 0.0, 3.0), (3.0, 0.0, 3.0), (3.0, 0.0, -3.0), (-3.0, 0.0, -3.0)]
FLOOR_T = [(0, 1, 2), (0, 2, 3)]
CAM = ((0.113, 3.021, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 24, 18)
ABOVE = ((0.3, 4.0, 0.5), (0.8, 0.8, 0.8))
BELOW = ((0.2, -50.0, 0.1), (0.5, 0.5, 0.6))


def octahedron(c, r):
    """Eight outward faces on shared vertices: PHONG normals are interpolated and not renormalised."""
    v = [(c[0] + r, c[1], c[2]), (c[0] - r, c[1], c[2]), (c[0], c[1] + r, c[2]), (c[0], c[1] - r, c[2]),
         (c[0], c[1], c[2] + r), (c[0], c[1], c[2] - r)]
    t = []
    for sx in (0, 1):
        for sy in (0, 1):
            for sz in (0, 1):
                x, y, z = sx, 2 + sy, 4 + sz
                even = (sx + sy + sz) % 2 == 0   # sign product > 0
                t.append((x, y, z) if even else (x, z, y))
    return v, t


def scenes():
    """name -> (meshes, lights, cam_def, background, ambience, max_depth)."""
    out = {}
    bg, amb = (0.05, 0.1, 0.2), (0.2, 0.2, 0.2)
    floor = lambda mat: minirt.Mesh(FLOOR_V, FLOOR_T, "FLAT", mat)  # noqa: E731
    # a floor facing up, one light above and one far below it
    out["floor_two_lights"] = ([floor(SHINY)], [ABOVE, BELOW], CAM, bg, amb, 1)
    # the same with shininess 0: the light below adds ks * pow(0, 0) = ks, nothing may be skipped
    out["floor_shininess_zero"] = ([floor(DULL)], [ABOVE, BELOW], CAM, bg, amb, 1)
    # the light below first (the owner's own ray), then the light above
    out["floor_below_first"] = ([floor(SHINY)], [BELOW, ABOVE], CAM, bg, amb, 1)
    # lights in the floor's plane and 1e-9 to either side of it (beyond the floor's edge), one above
    out["grazing"] = ([floor(SHINY)],
                      [((5.0, 0.0, 0.3), (0.5, 0.5, 0.5)), ((-5.0, 1e-9, 0.2), (0.4, 0.5, 0.4)),
                       ((0.4, -1e-9, 5.0), (0.5, 0.4, 0.4)), ABOVE], CAM, bg, amb, 1)
    # PHONG octahedron over the floor, lit from the side: n.l changes sign across its faces
    ov, ot = octahedron((0.0, 1.1, 0.0), 1.0)
    side = ((4.0, 1.3, 0.7), (0.8, 0.7, 0.6))
    out["phong_terminator"] = ([floor(SHINY), minirt.Mesh(ov, ot, "PHONG", SHINY)], [side, ABOVE], CAM, bg, amb, 1)
    out["one_light"] = ([floor(SHINY), minirt.Mesh(ov, ot, "PHONG", SHINY)], [side], CAM, bg, amb, 1)
    # a mirror floor with both lights below it, a coloured octahedron above to reflect: depth 3
    out["mirror_lights_behind"] = ([floor(MIRROR), minirt.Mesh(ov, ot, "FLAT", SHINY)],
                                   [BELOW, ((-1.0, -3.0, 0.5), (0.4, 0.4, 0.4))], CAM, bg, amb, 3)
    # 40 lights around the octahedron, every other one below the mirror floor: two shadow batches
    many = [((1.8 * ((i * 37) % 19 - 9) / 9.0, (2.5 + 0.05 * (i % 7)) * (1 if i % 2 == 0 else -1), 1.2 - 0.06 * i),
             (0.02 + 0.001 * (i % 11), 0.025, 0.03 - 0.0005 * (i % 5))) for i in range(40)]
    out["many_lights"] = ([floor(MIRROR), minirt.Mesh(ov, ot, "FLAT", SHINY)], many, CAM, bg, amb, 2)
    return out


def write(tmpdir, name, size=None):
    meshes, lights, cam_def, bg, amb, depth = scenes()[name]
    if size is not None:
        cam_def = cam_def[:4] + tuple(size)
    path = tmpdir / f"{name}.sce"
    minirt.write_sce(path, meshes, lights, cam_def, bg, amb, depth)
    return path


def mini(name):
    meshes, lights, cam_def, bg, amb, depth = scenes()[name]
    eye, center, up, fovy, w, h = cam_def
    return minirt.Scene(meshes, lights, minirt.camera(eye, center, up, fovy, w, h), bg, amb, depth)
