"""Scenes for the hierarchy-optimiser tests (rt_upload_options.tree_opt), shared by
tests/test_tree_opt_host.py (rt_debug_tree_report, no GPU) and tests/test_tree_opt_gpu.py.

tri1 .. tri4   one to four separate triangles: the root is a leaf; the root's children are leaves
               (no eligible node); with four, the root's grandchildren are the only eligible nodes.
coincident     the same triangle six times, three more in its plane: boxes that coincide exactly.
zero_area      triangles with collinear or repeated vertices on one axis-parallel line: every box
               of the hierarchy has surface area 0.
deep, flat, occluder, fan   tests/stack_fast_scenes.py (deep: the tunnel of 65536 slivers).
split_stress   the hostile scene of tests/test_gpu_parity.py's spatial-split test, rebuilt here: a
               fan of long thin triangles, crossing room-sized quads, zero-area triangles, a PHONG strip.
cornell        the generator's cornell box, detail 3.
random20k      20 000 random triangles (the generator's soup).
office         the office proxy.
"""
import math

import kat_scenes
import minirt
import stack_fast_scenes as sfs

MATT = sfs.MATT
LIGHTS = [((2.0, 3.0, 5.0), (0.7, 0.7, 0.65))]
CAM = ((0.1, 0.05, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, sfs.W, sfs.H)

HAND = ["tri1", "tri2", "tri3", "tri4", "coincident", "zero_area"]
GENERATED = {"cornell": ("cornell", {"detail": 3}), "random20k": ("random_tris", {"n_triangles": 20000}),
             "office": ("office", {})}
NAMES = HAND + sfs.NAMES + ["split_stress"] + list(GENERATED)
BY_SIZE_ON = {"deep", "cornell", "random20k", "office"}   # 2^10 <= triangles < 2^18: the default optimises them


def hand_triangles(name):
    if name.startswith("tri"):
        return sfs.flat_triangles()[:int(name[3:])]
    if name == "coincident":
        t = [(-1.0, -0.5, 0.0), (1.0, -0.5, 0.0), (0.0, 1.0, 0.0)]
        return [list(t) for _ in range(6)] + [[(x + 0.25, y, 0.0) for x, y, _ in t] for _ in range(3)]
    if name == "zero_area":   # all on the line y = 0.3, z = 0.1
        xs = [(-1.5, -0.5, 0.5), (0.2, 0.2, 1.1), (-0.7, -0.7, -0.7), (1.0, 1.4, 1.8), (-0.2, 0.9, 0.3)]
        return [[(x, 0.3, 0.1) for x in t] for t in xs]
    raise KeyError(name)


def split_stress(tmp_path):
    fan_v, fan_t = [(0.0, 0.0, 0.2)], []
    n = 120
    for i in range(n):
        a = 2 * math.pi * i / n
        fan_v.append((1.5 * math.cos(a), 0.9 * math.sin(a), 0.2 + 0.3 * math.cos(3 * a)))
    for i in range(n):
        fan_t.append((0, 1 + i, 1 + (i + 1) % n))
    wall_v = [(0.1, -2.0, -2.0), (0.1, 2.0, -2.0), (0.1, 2.0, 2.0), (0.1, -2.0, 2.0),
              (-2.0, -0.2, -2.0), (2.0, -0.2, -2.0), (2.0, -0.2, 2.0), (-2.0, -0.2, 2.0)]
    wall_t = [(0, 1, 2), (0, 2, 3), (4, 6, 5), (4, 7, 6)]
    deg_v = [(-0.5, 0.5, 0.5), (0.0, 0.5, 0.5), (0.5, 0.5, 0.5), (0.3, -0.4, 0.6), (0.3, -0.4, 0.6), (0.9, 0.2, 0.4)]
    deg_t = [(0, 1, 2), (3, 4, 5), (2, 1, 0)]
    mirror = ((0.05, 0.05, 0.05), (0.3, 0.3, 0.35), (0.5, 0.5, 0.5), 40.0, 0.4, 1)
    meshes = [minirt.Mesh(fan_v, fan_t, "FLAT", mirror), minirt.Mesh(wall_v, wall_t, "FLAT", kat_scenes.FLAT_MAT),
              minirt.Mesh(deg_v, deg_t, "FLAT", kat_scenes.FLAT_MAT)]
    meshes += kat_scenes.scenes()["phong"][0]
    lights = [((0.6, 1.4, 3.0), (0.7, 0.7, 0.7)), ((-1.2, -0.3, 2.5), (0.3, 0.35, 0.3))]
    cam = ((0.35, 0.62, 3.6), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, sfs.W, sfs.H)
    path = tmp_path / "split_stress.sce"
    minirt.write_sce(path, meshes, lights, cam, (0.05, 0.05, 0.1), (0.2, 0.2, 0.2), 3)
    return path


def write(name, tmp):
    """Writes the scene file of a scene that is not generated; returns its path."""
    if name in sfs.NAMES:
        return sfs.write(name, tmp)
    if name == "split_stress":
        return split_stress(tmp)
    path = tmp / f"{name}.sce"
    tris = hand_triangles(name)
    mesh = minirt.Mesh([v for t in tris for v in t], [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(len(tris))], "FLAT", MATT)
    minirt.write_sce(path, [mesh], LIGHTS, CAM, sfs.BG, sfs.AMB, 2)
    return path


_hosts = {}


def host(name, tmp_path_factory):
    """The prepared HostScene of scene `name`, made once per session."""
    import rtamd

    if name not in _hosts:
        if name in GENERATED:
            kind, gen = GENERATED[name]
            hs = rtamd.HostScene.generate(kind, **gen)
        else:
            hs = rtamd.HostScene.load(write(name, tmp_path_factory.mktemp(f"treeopt_{name}")))
        hs.prepare()
        _hosts[name] = hs
    return _hosts[name]


if __name__ == "__main__":   # the scene files, for tools/tree_opt_check.cpp
    import sys
    from pathlib import Path

    out = Path(sys.argv[1])
    out.mkdir(parents=True, exist_ok=True)
    for n in NAMES:
        if n not in GENERATED:
            print(write(n, out))
