"""Scenes for the traversal-stack tests: small fixed-seed frames at 64x48 whose
traversals stress the 4-wide node loop's stack pushes and pops.  Written as .sce/.obj and loaded
through the product loader, like tests/fetch_batch_scenes.py; tests/test_stack_fast_scenes.py pins
them on the CPU.

deep      a tunnel of DEEP_N triangles one behind the other along the view axis, each a sliver
          across the view cone's cross-section with a bounding box that is all of it.  Every box of every
          hierarchy over them contains every ray of the frame, so a ray meets all children of all
          nodes on its way down: the stack grows by up to three entries per 4-wide level, past
          RING - 3, RING and beyond for both ring sizes (8 and 16), then empties again through the
          spill array.  Half of the triangles face the eye and a light beside it, the others a light behind
          the tunnel's far end, whose shadow rays run through all of the tunnel.
flat      twelve separate triangles on a wall: two levels of 4-wide nodes, a stack of at most three.
occluder  a floor of small mirror and matt tents under two lights, and one large triangle that hides
          both lights from about half of the floor: tiles of the frame whose shadow rays are all occluded,
          tiles whose rays all reach the lights, and tiles with both; reflection rays (closest hit)
          share waves with shadow rays (any hit).
fan       four sparse lattices of small triangles at four depths, whose rectangles overlap in the
          middle of the view and leave its margins empty: primary rays meet 0, 1, 2, 3 and 4 of the
          four lattices' boxes.
"""
import random

import minirt

W, H = 64, 48
BG, AMB = (0.05, 0.1, 0.2), (0.2, 0.2, 0.2)

MATT = ((0.1, 0.1, 0.1), (0.7, 0.6, 0.5), (0.3, 0.3, 0.3), 20.0, 0.0, 1)
MIRROR = ((0.05, 0.05, 0.08), (0.3, 0.5, 0.6), (0.5, 0.5, 0.5), 40.0, 0.4, 1)

# ------------------------------------------------------------------ deep
DEEP_N = 65536
DEEP_Z0, DEEP_DZ = 10.0, 1.0 / 128.0   # distance of the first triangle from the eye, spacing
DEEP_FOVY = 10.0
DEEP_CAM = ((0.0, 0.0, 0.0), (0.0, 0.0, -DEEP_Z0), (0.0, 1.0, 0.0), DEEP_FOVY, W, H)
# one light beside the eye, one behind the tunnel's far end
DEEP_LIGHTS = [((0.07, 0.05, -0.5), (0.6, 0.6, 0.55)), ((-0.4, 0.3, -(DEEP_Z0 + DEEP_N * DEEP_DZ + 2.0)), (0.5, 0.5, 0.6))]


def deep_triangles():
    """Triangle k stands at z = -(Z0 + k DZ), across the axis: a sliver along one diagonal of the
    view cone's cross-section there -- two opposite corners, each pushed outwards by its own factor
    in [1.02, 1.12] (no two equal boxes), and a third vertex beside the diagonal, off it by 0.08 to
    1.0 of the half-width and out of the plane by up to 0.4 DZ (its own normal).  A ray passes a
    few slivers before it hits one."""
    rng = random.Random(20251)
    half_h = 0.0874886635259240   # tan(5 degrees): half the view's height at distance 1
    half_w = half_h * W / H
    tris = []
    for k in range(DEEP_N):
        d = DEEP_Z0 + k * DEEP_DZ
        sy = 1 if rng.random() < 0.5 else -1          # which diagonal: (-1, -sy) .. (1, sy)
        fa, fb = 1.02 + 0.1 * rng.random(), 1.02 + 0.1 * rng.random()
        u = -0.6 + 1.2 * rng.random()                   # along the diagonal
        off = (0.08 + 0.92 * rng.random()) * (1 if rng.random() < 0.5 else -1)
        dz = DEEP_DZ * (-0.4 + 0.8 * rng.random())
        tri = [(-half_w * d * fa, -sy * half_h * d * fa, -d), (half_w * d * fb, sy * half_h * d * fb, -d),
               ((u - off) * half_w * d, (u + off) * sy * half_h * d, -d + dz)]
        if rng.random() < 0.5:   # faces the far light instead of the eye
            tri.reverse()
        tris.append(tri)
    return tris


# ------------------------------------------------------------------ flat
FLAT_CAM = ((0.1, 0.05, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, W, H)
FLAT_LIGHTS = [((2.0, 3.0, 5.0), (0.7, 0.7, 0.65))]


def flat_triangles():
    tris = []
    for i in range(4):
        for j in range(3):
            x, y = -2.0 + 1.1 * i + 0.03 * j, -1.4 + 1.0 * j + 0.02 * i
            tris.append([(x, y, 0.1 * ((i + j) % 3)), (x + 0.8, y + 0.1, 0.0), (x + 0.3, y + 0.7, 0.05 * i)])
    return tris


# ------------------------------------------------------------------ occluder
OCC_CAM = ((0.137, 5.031, 6.017), (0.011, 0.0, 0.007), (0.0, 1.0, 0.0), 40.0, W, H)
OCC_LIGHTS = [((-6.0, 6.0, 1.0), (0.6, 0.6, 0.55)), ((-5.0, 7.0, -2.0), (0.35, 0.35, 0.4))]
OCC_NX, OCC_NZ = 16, 12


def occluder_triangles():
    """(matt tents, mirror tents, occluder): tents of four triangles on the floor y = 0; the occluder
    stands between the lights and the floor's x < 0 half."""
    rng = random.Random(20252)
    matt, mirror = [], []
    sx, sz = 8.0 / OCC_NX, 6.0 / OCC_NZ
    for i in range(OCC_NX):
        for j in range(OCC_NZ):
            x0, z0 = -4.0 + sx * i, -3.0 + sz * j
            apex = (x0 + sx * (0.4 + 0.2 * rng.random()), 0.05 + 0.1 * rng.random(), z0 + sz * (0.4 + 0.2 * rng.random()))
            base = [(x0, 0.0, z0), (x0, 0.0, z0 + sz), (x0 + sx, 0.0, z0 + sz), (x0 + sx, 0.0, z0)]
            out = mirror if (i + 2 * j) % 3 == 0 else matt
            out += [[base[k], base[(k + 1) % 4], apex] for k in range(4)]
    occluder = [[(-4.5, 0.2, -6.0), (-4.5, 0.2, 6.0), (-2.5, 5.0, 0.0)]]
    return matt, mirror, occluder


# ------------------------------------------------------------------ fan
FAN_CAM = ((0.03, 0.02, 8.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 30.0, W, H)
FAN_LIGHTS = [((3.0, 4.0, 9.0), (0.7, 0.7, 0.65))]
# lattice: (x range, y range, z); the view is about 5.7 x 4.3 at z = 0
FAN_RECTS = [((-2.0, 0.4), (-1.2, 1.2), 0.0), ((-0.4, 2.0), (-1.2, 1.2), -3.0),
             ((-1.2, 1.2), (-1.6, 0.3), -6.0), ((-1.2, 1.2), (-0.3, 1.6), -9.0)]
FAN_STEP = 0.3


def fan_triangles():
    """One list of triangles per lattice: small triangles on a grid of pitch FAN_STEP that cover about
    a fifth of it, so most rays pass a lattice's box without a hit."""
    rng = random.Random(20253)
    out = []
    for (xa, xb), (ya, yb), z in FAN_RECTS:
        tris = []
        nx, ny = round((xb - xa) / FAN_STEP), round((yb - ya) / FAN_STEP)
        for i in range(nx + 1):
            for j in range(ny + 1):
                # the lattice's corners are always occupied: its box is the rectangle
                x, y = xa + (xb - xa) * i / nx, ya + (yb - ya) * j / ny
                s = 0.1 + 0.05 * rng.random()
                tris.append([(x - s, y - s, z), (x + s, y - s, z + 0.02), (x, y + s, z - 0.02)])
        out.append(tris)
    return out


def fan_boxes():
    """[(lo, hi)] of the four lattices."""
    boxes = []
    for tris in fan_triangles():
        v = [p for t in tris for p in t]
        boxes.append((tuple(min(p[k] for p in v) for k in range(3)), tuple(max(p[k] for p in v) for k in range(3))))
    return boxes


# ------------------------------------------------------------------ writers
def _soup(tris, mode, mat):
    verts = [v for t in tris for v in t]
    return minirt.Mesh(verts, [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(len(tris))], mode, mat)


def scene(name):
    """(meshes, lights, camera, depth) of scene `name`."""
    if name == "deep":
        return [_soup(deep_triangles(), "FLAT", MIRROR)], DEEP_LIGHTS, DEEP_CAM, 2
    if name == "flat":
        return [_soup(flat_triangles(), "FLAT", MATT)], FLAT_LIGHTS, FLAT_CAM, 2
    if name == "occluder":
        matt, mirror, occ = occluder_triangles()
        return [_soup(matt, "FLAT", MATT), _soup(mirror, "PHONG", MIRROR), _soup(occ, "FLAT", MATT)], OCC_LIGHTS, OCC_CAM, 2
    if name == "fan":
        lat = fan_triangles()
        return [_soup(t, "FLAT", MIRROR if k == 0 else MATT) for k, t in enumerate(lat)], FAN_LIGHTS, FAN_CAM, 2
    raise KeyError(name)


NAMES = ["deep", "flat", "occluder", "fan"]


def write(name, tmpdir):
    path = tmpdir / f"{name}.sce"
    if name == "deep":   # 65536 triangles: written without minirt.Mesh's per-vertex normals
        _write_soup(path, deep_triangles(), MIRROR, DEEP_LIGHTS, DEEP_CAM, 2)
    else:
        meshes, lights, cam, depth = scene(name)
        minirt.write_sce(path, meshes, lights, cam, BG, AMB, depth)
    return path


def _write_soup(path, tris, mat, lights, cam, depth):
    r = lambda v: " ".join(repr(float(x)) for x in v)  # noqa: E731
    eye, center, up, fovy, w, h = cam
    obj = path.with_name(f"{path.stem}_m0.obj")
    with open(obj, "w") as f:
        f.write("".join(f"v {r(p)}\n" for t in tris for p in t))
        f.write("".join(f"f {3 * k + 1} {3 * k + 2} {3 * k + 3}\n" for k in range(len(tris))))
    ka, kd, ks, shin, mirror, sh = mat
    lines = [f"camera {r(eye)} {r(center)} {r(up)} {float(fovy)!r} {w} {h}", f"depth {depth}", f"background {r(BG)}",
             f"ambience {r(AMB)}"]
    lines += [f"light {r(lp)} {r(lc)}" for lp, lc in lights]
    lines.append(f"mesh {obj.name} FLAT {r(ka)} {r(kd)} {r(ks)} {float(shin)!r} {float(mirror)!r} {int(sh)}")
    path.write_text("\n".join(lines) + "\n")
