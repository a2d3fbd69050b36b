"""Scenes for the record-fetch tests: the leaf loop's triangle fetch and SHADE's
material fetch.  Written as .sce/.obj (+ .mtl/.ppm) and loaded through the product loader, like
tests/shadow_batch_scenes.py; tests/test_fetch_batch_scenes.py pins them on the CPU.

leaf      clusters of 1 .. 6 triangles that share one centroid, which the reference's median split
          cannot separate (leaves of 1 .. 5 and more records), some with a zero-area or a sliver
          triangle among them (|S| < 1e-10 for every ray), horizontal shelves (|S| < 1e-10 for the
          rays of the middle pixel row, whose direction is horizontal), a wall behind.  Clusters are
          about five pixels wide, so the lanes of an 8x8 tile sit in different leaves and take and
          skip the branch in one wave instruction.  Everything stands at y ~ 32, z ~ -64 with
          x in [-3, 3]: a wrong p2.y or p2.z moves the picture.
material  a wall of small tents, each about four pixels wide, that belong to seven meshes -- FLAT and
          PHONG, with and without a texture, shadowable or not, mirror or not -- laid out so that
          neighbouring tents are of different meshes, and a sphere (analytic primitive, its own
          material) in front of them.  Two lights, depth 3.
"""
import minirt

W, H = 64, 48
BG, AMB = (0.05, 0.1, 0.2), (0.2, 0.2, 0.2)
OY, OZ = 32.0, -64.0   # where the scenes stand

SHINY = ((0.1, 0.1, 0.1), (0.7, 0.6, 0.5), (0.3, 0.3, 0.3), 20.0, 0.0, 1)
GLOSS = ((0.05, 0.05, 0.08), (0.3, 0.5, 0.6), (0.5, 0.5, 0.5), 40.0, 0.4, 1)

# ------------------------------------------------------------------ leaf scene
LEAF_CAM = ((0.113, OY, OZ + 6.0), (0.0, OY, OZ), (0.0, 1.0, 0.0), 40.0, W, H)   # a horizontal view
LEAF_LIGHTS = [((2.5, OY + 3.0, OZ + 5.0), (0.6, 0.6, 0.55)), ((-3.0, OY + 1.0, OZ + 4.0), (0.35, 0.35, 0.4))]
NX, NY = 9, 7   # clusters


def _cluster(c, k, kind):
    """k ordinary triangles around centroid c (vertex offsets are dyadic and sum to zero, so the
    centroids are bit-equal), tilted differently so that they cross only along a line, plus one
    zero-area (kind 0) or sliver (kind 1) triangle with the same centroid."""
    tris = []
    for j in range(k):
        s = j / 32.0
        r = 1.0 - j / 16.0
        tris.append([(c[0] - 0.1875 * r, c[1] - 0.125 * r, c[2] + s), (c[0] + 0.1875 * r, c[1] - 0.125 * r, c[2] + s),
                     (c[0], c[1] + 0.25 * r, c[2] - 2.0 * s)])
    if kind == 0:     # collinear: e1 x e2 = 0 exactly
        tris.append([(c[0] - 0.125, c[1] - 0.0625, c[2]), (c[0], c[1], c[2]), (c[0] + 0.125, c[1] + 0.0625, c[2])])
    elif kind == 1:   # sliver: |e1 x e2| = 0.375 * 2^-40
        e = 2.0 ** -41
        tris.append([(c[0] - 0.125, c[1] - e, c[2]), (c[0] + 0.125, c[1] - e, c[2]), (c[0], c[1] + 2.0 * e, c[2])])
    return tris


def leaf_triangles():
    """(cluster triangles, shelf triangles, wall triangles); each a list of three vertices."""
    clusters = []
    for i in range(NX):
        for j in range(NY):
            n = i * NY + j
            # no two clusters share a coordinate: the median split separates them on every axis
            c = (-2.0 + 0.5 * i + j / 64.0, OY - 1.5 + 0.5 * j + i / 128.0 + 1.0 / 16.0, OZ + ((7 * i + 3 * j) % 16) / 64.0)
            clusters += _cluster(c, 1 + n % 6, n % 3)
    shelves = []
    for k, (x, y) in enumerate([(-1.3, OY - 0.8), (0.4, OY + 0.7), (1.6, OY - 0.3), (-0.2, OY + 1.2)]):
        z = OZ + 1.0 + 0.25 * k
        shelves.append([(x - 0.5, y, z + 0.4), (x + 0.5, y, z + 0.4), (x + 0.1 * k, y, z - 0.4)])
    wall = [[(-4.0, OY - 3.0, OZ - 2.0), (4.0, OY - 3.0, OZ - 2.0), (4.0, OY + 3.0, OZ - 2.0)],
            [(-4.0, OY - 3.0, OZ - 2.0), (4.0, OY + 3.0, OZ - 2.0), (-4.0, OY + 3.0, OZ - 2.0)]]
    return clusters, shelves, wall


def _soup(tris, mode, mat):
    verts = [v for t in tris for v in t]
    return minirt.Mesh(verts, [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(len(tris))], mode, mat)


def leaf_scene():
    clusters, shelves, wall = leaf_triangles()
    meshes = [_soup(clusters, "FLAT", GLOSS), _soup(shelves, "FLAT", SHINY), _soup(wall, "PHONG", SHINY)]
    return meshes, LEAF_LIGHTS, LEAF_CAM, BG, AMB, 2


# ------------------------------------------------------------------ material scene
# name: (mode, textured, (ka, kd, ks, shininess, mirror, shadowable))
KINDS = {
    "flat": ("FLAT", False, ((0.1, 0.1, 0.1), (0.7, 0.6, 0.5), (0.3, 0.3, 0.3), 20.0, 0.0, 1)),
    "phong_mirror": ("PHONG", False, ((0.05, 0.05, 0.05), (0.2, 0.3, 0.6), (0.5, 0.5, 0.5), 40.0, 0.5, 1)),
    "flat_tex": ("FLAT", True, ((0.1, 0.1, 0.1), (1.0, 1.0, 1.0), (0.2, 0.2, 0.2), 12.0, 0.0, 1)),
    "phong_tex_unshadowed": ("PHONG", True, ((0.15, 0.1, 0.1), (1.0, 1.0, 1.0), (0.3, 0.3, 0.3), 8.0, 0.0, 0)),
    "flat_mirror_unshadowed": ("FLAT", False, ((0.02, 0.05, 0.02), (0.3, 0.6, 0.3), (0.4, 0.4, 0.4), 30.0, 0.35, 0)),
    "phong_unshadowed": ("PHONG", False, ((0.1, 0.05, 0.1), (0.6, 0.3, 0.6), (0.25, 0.25, 0.25), 16.0, 0.0, 0)),
    "flat_tex_mirror": ("FLAT", True, ((0.05, 0.05, 0.05), (1.0, 1.0, 1.0), (0.3, 0.3, 0.3), 25.0, 0.3, 1)),
}
SPHERE = ((0.45, OY + 0.3, OZ + 1.6), 0.6, ((0.05, 0.02, 0.02), (0.7, 0.25, 0.2), (0.6, 0.6, 0.6), 50.0, 0.3, 1))
MAT_CAM = ((0.113, OY + 0.2, OZ + 6.0), (0.0, OY, OZ), (0.0, 1.0, 0.0), 40.0, W, H)
MAT_LIGHTS = [((2.5, OY + 3.0, OZ + 5.0), (0.6, 0.6, 0.55)), ((-3.0, OY - 1.0, OZ + 4.5), (0.35, 0.35, 0.4))]
TX, TY = 20, 15   # tents across the view (the view is about 5.8 x 4.4 at the wall)
TEX_W, TEX_H = 7, 5


def tent_meshes():
    """name -> (vertices, triangles, uv): a tent is four triangles around an apex that stands out of
    the wall (vertex normals differ across it); tent (i, j) belongs to kind (i + 3 j) mod 7."""
    names = list(KINDS)
    out = {n: ([], [], []) for n in names}
    sx, sy = 6.0 / TX, 4.6 / TY
    for i in range(TX):
        for j in range(TY):
            v, t, uv = out[names[(i + 3 * j) % len(names)]]
            x0, y0 = -3.07 + sx * i, OY - 2.33 + sy * j   # (no tent edge on the view's axes)
            b = len(v)
            h = 0.08 + 0.01 * ((i + j) % 5)
            v += [(x0, y0, OZ), (x0 + sx, y0, OZ), (x0 + sx, y0 + sy, OZ), (x0, y0 + sy, OZ),
                  (x0 + 0.5 * sx, y0 + 0.5 * sy, OZ + h)]
            uv += [(0.1 * (i % 9), 0.1 * (j % 7)), (0.1 * (i % 9) + 0.35, 0.1 * (j % 7)),
                   (0.1 * (i % 9) + 0.35, 0.1 * (j % 7) + 0.4), (0.1 * (i % 9), 0.1 * (j % 7) + 0.4),
                   (0.1 * (i % 9) + 0.17, 0.1 * (j % 7) + 0.21)]
            t += [(b, b + 1, b + 4), (b + 1, b + 2, b + 4), (b + 2, b + 3, b + 4), (b + 3, b, b + 4)]
    return out


def texture_bytes(k):
    return bytes((37 * x + 91 * y + 53 * c + 29 * k) % 256 for y in range(TEX_H) for x in range(TEX_W) for c in range(3))


def _r(v):
    return " ".join(repr(float(x)) for x in v)


def _mat_line(mat):
    ka, kd, ks, shin, mirror, sh = mat
    return f"{_r(ka)} {_r(kd)} {_r(ks)} {float(shin)!r} {float(mirror)!r} {int(sh)}"


def write_material(tmpdir, size=None):
    w, h = size or (W, H)
    eye, center, up, fovy = MAT_CAM[:4]
    path = tmpdir / "material.sce"
    lines = [f"camera {_r(eye)} {_r(center)} {_r(up)} {float(fovy)!r} {w} {h}", "depth 3", f"background {_r(BG)}",
             f"ambience {_r(AMB)}"]
    lines += [f"light {_r(p)} {_r(c)}" for p, c in MAT_LIGHTS]
    for k, (name, (verts, tris, uv)) in enumerate(tent_meshes().items()):
        mode, textured, mat = KINDS[name]
        obj = [f"v {_r(v)}" for v in verts]
        if textured:
            (tmpdir / f"material_{name}.ppm").write_bytes(f"P6\n{TEX_W} {TEX_H}\n255\n".encode() + texture_bytes(k))
            (tmpdir / f"material_{name}.mtl").write_text(f"newmtl tex\nKd 1 1 1\nmap_Kd material_{name}.ppm\n")
            obj = [f"mtllib material_{name}.mtl"] + obj + [f"vt {_r(t)}" for t in uv] + ["usemtl tex"]
            obj += ["f " + " ".join(f"{i + 1}/{i + 1}" for i in t) for t in tris]
        else:
            obj += ["f " + " ".join(str(i + 1) for i in t) for t in tris]
        (tmpdir / f"material_{name}.obj").write_text("\n".join(obj) + "\n")
        lines.append(f"mesh material_{name}.obj {mode} {_mat_line(mat)}")
    c, r, mat = SPHERE
    lines.append(f"sphere {_r(c)} {float(r)!r} {_mat_line(mat)}")
    path.write_text("\n".join(lines) + "\n")
    return path


def write_leaf(tmpdir, size=None):
    meshes, lights, cam, bg, amb, depth = leaf_scene()
    if size is not None:
        cam = cam[:4] + tuple(size)
    path = tmpdir / "leaf.sce"
    minirt.write_sce(path, meshes, lights, cam, bg, amb, depth)
    return path


def mini_leaf(size=None):
    meshes, lights, cam, bg, amb, depth = leaf_scene()
    eye, center, up, fovy, w, h = cam[:4] + tuple(size or (W, H))
    return minirt.Scene(meshes, lights, minirt.camera(eye, center, up, fovy, w, h), bg, amb, depth)
