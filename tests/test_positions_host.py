"""rt_normals_host and rt_host_slot_triangles on the host only -- no GPU, no HIP call.

rt_normals_host runs the CSR build and the per-thread bodies of the normal kernels of
rt_scene_update_positions.  Its vertex and face normals equal, byte for byte, the arrays
rt_host_update_vertices leaves in the SoA: on fuzz seeds 0-7 moved to B, on office and cornell with
the odd meshes moved, and on positions_cases' `fan` and `degenerate`, whose edge cases the first
test shows to have survived the loader (the unreferenced vertex, the repeated id, the zero-area
triangle, the skipped corner).  slot_triangles() is a permutation that update_vertices leaves alone
and that maps the SoA's face normals back to mesh order consistently with vertex_idx."""
import numpy as np
import pytest

import fuzz_scenes
import minirt
import positions_cases as pc
import rtamd
import scale_scenes as ss
import update_cases as uc


def _check(hs, pos):
    """rt_normals_host(pos) against the arrays update_vertices(pos) leaves."""
    vn, fn = pc.normals_host(hs, pos)
    hs.update_vertices(pos)
    soa = hs.soa_arrays()
    assert np.array_equal(pc.bits(vn), pc.bits(soa["vertex_normals"]))
    assert np.array_equal(pc.bits(fn), pc.bits(soa["face_normals"]))
    return vn, fn


def test_loader_keeps_the_edge_cases():
    hs = pc.load("fan")
    soa = hs.soa_arrays()
    lone = pc.unreferenced(hs)
    assert len(lone) == 1 and tuple(soa["vertex_pos"][lone[0]]) == pc.FAN_LONER
    assert np.abs(soa["vertex_pos"]).max() == -soa["vertex_pos"][lone[0], 0]          # it decides delta
    assert np.bincount(soa["vertex_idx"].reshape(-1)).max() == pc.FAN_N > 64          # the apex
    assert -pc.pos_b(hs, "fan")[lone[0], 0] == np.abs(pc.pos_b(hs, "fan")).max()
    hs = pc.load("degenerate")
    soa = hs.soa_arrays()
    base = int(np.flatnonzero(soa["vertex_mesh_id"] == 1)[0])
    tris = {tuple(int(v) - base for v in t) for t in soa["vertex_idx"]}
    assert {pc.ODD_TWICE, pc.ODD_COLLINEAR, pc.ODD_THIN} <= tris
    for P in (soa["vertex_pos"], pc.pos_b(hs, "degenerate")):
        odd = P[base:]
        w = pc.corner_weights(odd, pc.ODD_THIN)
        print("thin triangle's corner weights", w)
        assert 0.0 < abs(w[0]) <= pc.EPS and min(abs(w[1]), abs(w[2])) > pc.EPS
        p0, p1, p2 = (tuple(odd[i]) for i in pc.ODD_COLLINEAR)
        assert minirt.cross(minirt.sub(p1, p0), minirt.sub(p2, p0)) == (0.0, 0.0, 0.0)
        assert pc.corner_weights(odd, pc.ODD_COLLINEAR)[1] == 0.0
        p0, p1, p2 = (tuple(odd[i]) for i in pc.ODD_THIN)
        assert minirt.cross(minirt.sub(p1, p0), minirt.sub(p2, p0)) != (0.0, 0.0, 0.0)


@pytest.mark.parametrize("seed", uc.SEEDS)
def test_fuzz_scene_moved_to_b(seed):
    hs, _ = ss.load(fuzz_scenes.scene(seed, uc.W, uc.H))
    old = hs.soa_arrays()["vertex_normals"].copy()
    vn, _ = _check(hs, uc.pos_b(seed))
    assert not np.array_equal(vn, old)
    assert np.allclose(np.sqrt((vn * vn).sum(axis=1)), 1.0)


@pytest.mark.parametrize("name", uc.GENERATED)
def test_generated_scene_with_odd_meshes_moved(name):
    hs = uc.generated(name)
    soa = hs.soa_arrays()
    vn0, fn0 = pc.normals_host(hs, soa["vertex_pos"])       # the prepared scene's own normals too
    assert np.array_equal(pc.bits(vn0), pc.bits(soa["vertex_normals"]))
    assert np.array_equal(pc.bits(fn0), pc.bits(soa["face_normals"]))
    _check(hs, uc.generated_pos_b(hs))


@pytest.mark.parametrize("name", pc.MADE)
def test_made_scene(name):
    hs = pc.load(name)
    vn, fn = _check(hs, pc.pos_b(hs, name))
    soa = hs.soa_arrays()
    lone = pc.unreferenced(hs)
    assert np.array_equal(pc.bits(vn[lone]), np.zeros((len(lone), 3), dtype=np.uint64))   # (+0, +0, +0)
    if name == "degenerate":
        base = int(np.flatnonzero(soa["vertex_mesh_id"] == 1)[0])
        slot = {tuple(int(v) - base for v in t): s for s, t in enumerate(soa["vertex_idx"])}
        assert np.array_equal(fn[slot[pc.ODD_COLLINEAR]], np.zeros(3))    # the cross product itself
        assert np.array_equal(fn[slot[pc.ODD_TWICE]], np.zeros(3))
        assert np.isfinite(vn).all() and np.isfinite(fn).all()


@pytest.mark.parametrize("key", [("fuzz", uc.KEPT[0]), ("gen", "cornell"), ("made", "fan")])
def test_slot_triangles(key):
    hs, posB = pc.case(key)
    order = hs.slot_triangles()
    soa = hs.soa_arrays()
    nt = len(soa["vertex_idx"])
    assert order.dtype == np.int32 and order.shape == (nt,)
    assert np.array_equal(np.sort(order), np.arange(nt))
    assert not np.array_equal(order, np.arange(nt))          # the median split did permute
    # mesh order: the triangles of every mesh in its own order, rebased vertex ids
    raw = hs.raw.contents
    mesh_tris, vbase = [], 0
    for m in range(raw.n_meshes):
        rm = raw.meshes[m]
        mesh_tris.append(np.ctypeslib.as_array(rm.tri_vertex, shape=(rm.n_triangles, 3)) + vbase)
        vbase += rm.n_vertices
    mesh_tris = np.concatenate(mesh_tris)
    assert np.array_equal(soa["vertex_idx"], mesh_tris[order])
    # ... and the face normals, recomputed in mesh order by the pure-Python restatement
    P = soa["vertex_pos"]
    for s in range(0, nt, max(1, nt // 64)):
        a, b, c = (tuple(P[i]) for i in mesh_tris[order[s]])
        n = minirt.normalize(minirt.cross(minirt.sub(b, a), minirt.sub(c, a)))
        assert tuple(soa["face_normals"][s]) == n
    hs.update_vertices(posB)
    assert np.array_equal(hs.slot_triangles(), order)


def test_normals_host_errors():
    lib = rtamd.hip_lib()
    hs = pc.load("degenerate")
    soa = hs.soa_arrays()
    import ctypes as C
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    vidx, order, P = soa["vertex_idx"].copy(), hs.slot_triangles(), soa["vertex_pos"].copy()
    nv, nt = len(P), len(vidx)
    vn, fn = np.zeros((nv, 3)), np.zeros((nt, 3))

    def call(vidx=vidx, order=order, nv=nv, nt=nt, P=P, vn=vn, fn=fn):
        ptr = lambda a, t: a.ctypes.data_as(t) if a is not None else None  # noqa: E731
        return lib.rt_normals_host(ptr(vidx, ip), ptr(order, ip), nv, nt, ptr(P, dp), ptr(vn, dp), ptr(fn, dp))

    assert call() == rtamd.abi.RT_OK
    for kw in ({"vidx": None}, {"order": None}, {"P": None}, {"vn": None}, {"fn": None}, {"nv": -1}, {"nt": -1}):
        assert call(**kw) == rtamd.abi.RT_ERR_INVALID, kw
    twice = order.copy()
    twice[1] = twice[0]
    assert call(order=twice) == rtamd.abi.RT_ERR_INVALID and b"permutation" in lib.rt_last_error()
    far = order.copy()
    far[0] = nt
    assert call(order=far) == rtamd.abi.RT_ERR_INVALID
    bad = vidx.copy()
    bad[2, 1] = nv
    assert call(vidx=bad) == rtamd.abi.RT_ERR_INVALID and b"vertex id" in lib.rt_last_error()
    assert call(nv=0, nt=0, vidx=None, order=None, P=None, vn=None, fn=None) == rtamd.abi.RT_OK
