"""rt_scene_update_vertices on the device (include/rt_hip.h): vertices moved on the
uploaded topology, records rewritten and the 4-wide hierarchy refitted by kernels.  The moved scenes
are tests/update_cases.py's; tests/test_update_host.py holds their host side and non-vacuity.

  1. against a fresh upload of the updated host scene: frames, ray counts and query rows with ==;
  2. against the oracle on B = 2^10 A and 2^-10 A (same tree and slots: the test asserts it), fp64
     frames within 1e-12 and exact ray counts, the suite's own standard;
  3. against brute force over all triangles, independent of any tree: t with ==;
  4. round trip A -> B -> A: with tree "sah" the device's nodes, triangle and normal records are
     byte-identical to the upload's; with "sbvh" every box contains the upload's;
  5. edges: a leaf root, both node numberings, device bytes, the canonical counters, the coordinate
     limit, updates and renders queued on one stream."""
import ctypes as C

import numpy as np
import pytest

import kat_scenes
import query_cases as qc
import radiance_cases as rc
import rtamd
import scale_scenes as ss
import update_cases as uc
from rtamd import abi

pytestmark = pytest.mark.gpu

TOL64 = 1e-12
TREES = ("sbvh", "sah")
GW, GH = 64, 36          # frames of the generated scenes


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    return gpu_available


def _params(hs, w=0, h=0, spp=1, flags=0):
    p = hs.render_params(w, h, spp)
    p.out_format = rtamd.RT_OUT_RGB_F64
    p.flags = flags
    return p


def _rays(hs):
    P = hs.soa_arrays()["vertex_pos"]
    return np.concatenate([qc.random_rays(hs, 512), qc.vertex_rays(hs, P, 512)])


def _same_hits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("t", "alpha", "beta", "normal", "slot", "mesh", "prim"))


def _check_against_fresh(dev, hs, p, tree=None, **options):
    """The updated device scene against a fresh upload of the (updated) host scene: frame, ray counts
    and the rows of both queries, all with ==.  Returns the frame."""
    fresh = rtamd.DeviceScene(hs, 0, tree=tree, **options)
    img, st = dev.render(p)
    want, wst = fresh.render(p)
    assert np.array_equal(img, want)
    assert rc.counts(st) == rc.counts(wst) and st.pixels == wst.pixels
    rays = _rays(hs)
    got, qs = dev.trace(rays, stats=True)
    ref, rs = fresh.trace(rays, stats=True)
    assert _same_hits(got, ref) and qs.hits == rs.hits and qs.watchdog == 0
    assert np.array_equal(dev.trace(rays, occluded=True), fresh.trace(rays, occluded=True))
    assert rs.hits >= 64
    lo, hi = dev.bounds()
    flo, fhi = fresh.bounds()
    assert np.array_equal(lo, flo) and np.array_equal(hi, fhi)
    fresh.close()
    return img


# ---- 1. against a fresh upload ----
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("seed", uc.KEPT)
def test_updated_fuzz_scene_equals_fresh_upload(seed, tree):
    hsA, _ = uc.fuzz_a(seed)
    hsU = uc.updated(seed)
    dev = rtamd.DeviceScene(hsA, 0, tree=tree)
    pA = _params(hsA)
    before, _ = dev.render(pA)
    dev.update(hsU)
    img = _check_against_fresh(dev, hsU, _params(hsU, spp=2 if seed == uc.KEPT[-1] else 1), tree=tree)
    if seed != uc.KEPT[-1]:
        assert not np.array_equal(img, before)   # the scene did move in the view
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 2
    dev.close()


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", uc.GENERATED)
def test_updated_generated_scene_equals_fresh_upload(name, tree):
    hs = uc.generated(name)
    dev = rtamd.DeviceScene(hs, 0, tree=tree)
    p = _params(hs, GW, GH)
    before, _ = dev.render(p)
    hs.update_vertices(uc.generated_pos_b(hs))
    dev.update(hs)
    img = _check_against_fresh(dev, hs, p, tree=tree)
    assert not np.array_equal(img, before)
    dev.close()


def test_fans_and_camera_points_equal_fresh_upload():
    seed = uc.KEPT[0]
    hsA, _ = uc.fuzz_a(seed)
    hsU = uc.updated(seed)
    dev = rtamd.DeviceScene(hsA, 0)
    dev.update(hsU)
    fresh = rtamd.DeviceScene(hsU, 0)
    p = _params(hsU)
    a, b = dev.camera(p, hits=True, points=True), fresh.camera(p, hits=True, points=True)
    pts = b["points"].cpu().numpy()
    assert _same_hits({k: v.cpu().numpy() for k, v in a["hits"].items()},
                      {k: v.cpu().numpy() for k, v in b["hits"].items()})
    assert np.array_equal(a["points"].cpu().numpy(), pts, equal_nan=True)
    assert np.isfinite(b["hits"]["t"].cpu().numpy()).sum() >= uc.MIN_HIT_FRACTION * uc.W * uc.H
    lo, hi = fresh.bounds()
    pts[:, 6] = 0.5 * float(np.sqrt(((hi - lo) ** 2).sum()))
    dirs = rtamd.ao_directions(8, 5, seed=1)
    want = fresh.ao(pts, dirs, seed=3, bias=1e-6)
    assert np.array_equal(dev.ao(pts, dirs, seed=3, bias=1e-6), want)
    assert np.any((want > 0) & (want < 8))
    pg = rc.params(hsU, 8, 8)
    gw, gst = fresh.gather(pts, dirs, pg, seed=3, bias=1e-6, stats=True)
    gg, st = dev.gather(pts, dirs, pg, seed=3, bias=1e-6, stats=True)
    assert np.array_equal(gg, gw) and rc.counts(st) == rc.counts(gst)
    assert len(np.unique(gw, axis=0)) >= 2
    dev.close()
    fresh.close()


# ---- 2. against the oracle, ties included ----
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("tname", ["x2^10", "x2^-10"])
def test_scaled_update_matches_oracle(tname, seed):
    keyA, keyB = ss.fuzz_key("identity", seed), ss.fuzz_key(tname, seed)
    (hsA, orcA), (hsB, orcB) = ss.case(keyA), ss.case(keyB)
    # the condition: power-of-two scaling keeps every comparison of the median split
    assert np.array_equal(orcA.bvh()["perm"], orcB.bvh()["perm"])
    assert np.array_equal(hsA.soa_arrays()["vertex_idx"], hsB.soa_arrays()["vertex_idx"])
    spp = ss.spp_of(seed)
    ref, cnt = ss.frame(keyB, spp, ss.REF)
    for tree in TREES:
        dev = rtamd.DeviceScene(hsA, 0, tree=tree)
        n4 = dev.debug_scene_image("nodes4")
        dev.update(hsB)
        img, st = dev.render(_params(hsB, spp=spp))
        err = float(np.abs(img - ref).max())
        print(f"{tname} seed {seed} {tree}: max |gpu - oracle| {err:.3e}, rays {rc.counts(st)}")
        assert err <= TOL64
        assert rc.counts(st) == ss.rays_counted(cnt)
        # delta changed by 2^10: every bound of every occupied slot must have moved
        m4 = dev.debug_scene_image("nodes4")
        occupied = n4[:, 24:28] != 0x7fffffff   # [node, slot]: not kEmpty
        for w in range(0, 24, 4):               # lo / hi of x, y, z: four slots each
            assert np.all((n4[:, w:w + 4] != m4[:, w:w + 4])[occupied])
            assert np.array_equal(n4[:, w:w + 4][~occupied], m4[:, w:w + 4][~occupied])
        assert np.array_equal(n4[:, 24:], m4[:, 24:])
        dev.close()
    assert cnt.closest_hits > 0


# ---- 3. against brute force ----
@pytest.mark.parametrize("seed", uc.KEPT[:2])
def test_updated_scene_matches_brute_force(seed):
    hsA, _ = uc.fuzz_a(seed)
    hsU = uc.updated(seed)
    rays = qc.vertex_rays(hsU, hsU.soa_arrays()["vertex_pos"], 256)
    want = ss.brute_force_t(hsU, rays)
    assert 64 <= np.isfinite(want).sum()
    for tree in TREES:
        dev = rtamd.DeviceScene(hsA, 0, tree=tree)
        dev.update(hsU)
        assert np.array_equal(dev.trace(rays)["t"], want), tree
        dev.close()


# ---- 4. round trip ----
def _round_trip(hsA, posA, posB, tree, **options):
    dev = rtamd.DeviceScene(hsA, 0, tree=tree, **options)
    first = {k: dev.debug_scene_image(k) for k in ("nodes4", "tris", "tnorm")}
    frame, _ = dev.render(_params(hsA, GW, GH))
    hs = hsA
    for pos in (posB, posA):
        hs.update_vertices(pos)
        dev.update(hs)
    again = {k: dev.debug_scene_image(k) for k in ("nodes4", "tris", "tnorm")}
    frame2, _ = dev.render(_params(hsA, GW, GH))
    dev.close()
    return first, again, frame, frame2


@pytest.mark.parametrize("name", ["fuzz", "cornell"])
def test_round_trip_sah_is_byte_identical(name):
    if name == "fuzz":
        seed = uc.KEPT[0]
        hs, _ = ss.load(uc.fuzz_scenes.scene(seed, uc.W, uc.H))
        posB = uc.pos_b(seed)
    else:
        hs = uc.generated(name)
        posB = uc.generated_pos_b(hs)
    posA = hs.soa_arrays()["vertex_pos"].copy()
    for options in ({"tree": "sah"}, {"tree": None}):   # default options: the byte test holds for the records
        first, again, f1, f2 = _round_trip(hs, posA, posB, **options)
        assert np.array_equal(first["tris"], again["tris"])
        assert np.array_equal(first["tnorm"].view(np.uint64), again["tnorm"].view(np.uint64))
        assert np.array_equal(f1, f2)
        if options["tree"] == "sah":
            assert np.array_equal(first["nodes4"], again["nodes4"])
        else:
            _assert_contains(again["nodes4"], first["nodes4"])


def _assert_contains(outer, inner):
    """Every box of `outer` contains the same slot's box of `inner`; refs and pad identical."""
    assert np.array_equal(outer[:, 24:], inner[:, 24:])
    of, nf = outer[:, :24].view(np.float32), inner[:, :24].view(np.float32)
    for a in range(3):
        lo_o, hi_o = of[:, 8 * a:8 * a + 4], of[:, 8 * a + 4:8 * a + 8]
        lo_i, hi_i = nf[:, 8 * a:8 * a + 4], nf[:, 8 * a + 4:8 * a + 8]
        assert np.all(lo_o <= lo_i) and np.all(hi_o >= hi_i)


# ---- 5. edges ----
def test_leaf_root_keeps_its_empty_slots(tmp_path):
    hs = rtamd.HostScene.load(kat_scenes.write(tmp_path, "one_tri"))
    hs.prepare()
    dev = rtamd.DeviceScene(hs, 0)
    P = hs.soa_arrays()["vertex_pos"].copy()
    P += np.array([0.2, -0.1, 0.3])
    P[0] += np.array([0.05, 0.02, -0.04])
    hs.update_vertices(P)
    dev.update(hs)
    n4 = dev.debug_scene_image("nodes4")
    assert len(n4) == 1
    f = n4[:, :24].view(np.float32)[0]
    assert np.array_equal(n4[0, 24:28], [0x80000000, 0x7fffffff, 0x7fffffff, 0x7fffffff])
    for a in range(3):
        assert np.all(f[8 * a + 1:8 * a + 4] == np.inf) and np.all(f[8 * a + 5:8 * a + 8] == -np.inf)
        assert np.isfinite(f[8 * a]) and np.isfinite(f[8 * a + 4])
    p = _params(hs)
    fresh = rtamd.DeviceScene(hs, 0)
    img, st = dev.render(p)
    want, wst = fresh.render(p)
    assert np.array_equal(img, want) and rc.counts(st) == rc.counts(wst)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) >= 2
    rays = qc.vertex_rays(hs, P, 128)
    assert _same_hits(dev.trace(rays), fresh.trace(rays))
    dev.close()
    fresh.close()


@pytest.mark.parametrize("treelet", [-1, 0])
def test_both_node_numberings(treelet):
    hs = uc.generated("cornell")
    assert 2000 <= hs.triangle_count <= 10000
    dev = rtamd.DeviceScene(hs, 0, lds_treelet=treelet)
    hs.update_vertices(uc.generated_pos_b(hs))
    dev.update(hs)
    _check_against_fresh(dev, hs, _params(hs, GW, GH), lds_treelet=treelet)
    dev.close()


def test_identity_update_and_device_bytes():
    hs = uc.generated("cornell")
    dev = rtamd.DeviceScene(hs, 0)
    p = _params(hs, GW, GH)
    img, st = dev.render(p)
    b0 = dev.device_bytes
    dev.update(hs)
    b1 = dev.device_bytes
    s = hs.soa.contents
    nt = s.n_vertex_idx // 3
    n4 = len(dev.debug_scene_image("nodes4"))
    assert b1 - b0 == 2 * 24 * s.n_vertices + 24 * nt + 4 * n4   # the three arrays and the schedule
    img1, st1 = dev.render(p)
    dev.update(hs)
    assert dev.device_bytes == b1
    img2, st2 = dev.render(p)
    assert np.array_equal(img1, img) and np.array_equal(img2, img)
    assert rc.counts(st1) == rc.counts(st) and rc.counts(st2) == rc.counts(st)
    dev.close()


def test_canonical_counters_are_refused_after_an_update():
    hs = uc.generated("cornell")
    dev = rtamd.DeviceScene(hs, 0)
    p = _params(hs, GW, GH, flags=rtamd.RT_FLAG_TRAVERSAL_STATS)
    _, st = dev.render(p)
    assert st.node_visits > 0 and st.tri_tests > 0
    dev.update(hs)
    img = np.zeros((GH, GW, 3))
    st = abi.Stats()
    lib = rtamd.hip_lib()
    assert lib.rt_render_to_host(dev._h, C.byref(p), img.ctypes.data_as(C.c_void_p), C.byref(st)) == abi.RT_ERR_UNSUPPORTED
    assert b"RT_FLAG_TRAVERSAL_STATS" in lib.rt_last_error()
    _, wide = dev.render(_params(hs, GW, GH, flags=rtamd.RT_FLAG_WIDE_STATS))
    assert wide.node_visits > 0 and wide.tri_tests > 0
    dev.close()


def test_coordinate_beyond_the_range_is_refused_and_changes_nothing():
    hs = uc.generated("cornell")
    dev = rtamd.DeviceScene(hs, 0)
    p = _params(hs, GW, GH)
    img, st = dev.render(p)
    b0, bounds0 = dev.device_bytes, dev.bounds()
    soa = hs.soa_arrays()
    P = soa["vertex_pos"].copy()
    P[3, 1] = 2.0 * abi.RT_MAX_COORDINATE
    with pytest.raises(rtamd.RtError, match="coordinate"):
        dev.update_vertices(P, soa["vertex_normals"], soa["face_normals"])
    lib = rtamd.hip_lib()
    dp = C.POINTER(C.c_double)
    u = abi.SceneUpdate(n_vertices=len(P), n_triangles=len(soa["face_normals"]), vertex_pos=P.ctypes.data_as(dp),
                        vertex_normals=soa["vertex_normals"].ctypes.data_as(dp),
                        face_normals=soa["face_normals"].ctypes.data_as(dp))
    assert lib.rt_scene_update_vertices(dev._h, C.byref(u), None) == abi.RT_ERR_UNSUPPORTED
    u.n_vertices += 1
    assert lib.rt_scene_update_vertices(dev._h, C.byref(u), None) == abi.RT_ERR_INVALID
    u.n_vertices -= 1
    u.n_triangles -= 1
    assert lib.rt_scene_update_vertices(dev._h, C.byref(u), None) == abi.RT_ERR_INVALID
    img2, st2 = dev.render(p)
    assert np.array_equal(img2, img) and rc.counts(st2) == rc.counts(st)
    assert dev.device_bytes == b0
    assert all(np.array_equal(a, b) for a, b in zip(dev.bounds(), bounds0))
    P[3, 1] = abi.RT_MAX_COORDINATE   # the limit itself is taken
    dev.update_vertices(P, soa["vertex_normals"], soa["face_normals"])
    dev.close()


def test_update_follows_the_launches_onto_the_cu_masked_stream():
    # reserve_cus: launches run on the caller's internal CU-masked stream; the update must run there
    # too, between the two frames, and the caller's stream must wait for it (the query runs on it)
    import torch

    hs = uc.generated("cornell")
    posA = hs.soa_arrays()["vertex_pos"].copy()
    dev = rtamd.DeviceScene(hs, 0, tree="sah", reserve_cus=32)
    p = _params(hs, GW, GH)
    outs = [torch.zeros((GH, GW, 3), dtype=torch.float64, device="cuda:0") for _ in range(2)]
    rays = torch.from_numpy(_rays(hs)).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    dev.launch(p, outs[0].data_ptr(), stream=stream.cuda_stream)
    hs.update_vertices(uc.generated_pos_b(hs))
    dev.update(hs, stream=stream.cuda_stream)
    dev.launch(p, outs[1].data_ptr(), stream=stream.cuda_stream)
    hits = dev.trace(rays, stream=stream.cuda_stream)
    stream.synchronize()
    got = [o.cpu().numpy() for o in outs]
    hits = {k: v.cpu().numpy() for k, v in hits.items()}
    fresh = rtamd.DeviceScene(hs, 0, tree="sah")
    assert np.array_equal(got[1], fresh.render(p)[0])
    assert _same_hits(hits, {k: v.cpu().numpy() for k, v in fresh.trace(rays).items()})
    fresh.close()
    hs.update_vertices(posA)
    first = rtamd.DeviceScene(hs, 0, tree="sah")
    assert np.array_equal(got[0], first.render(p)[0]) and not np.array_equal(got[0], got[1])
    first.close()
    dev.close()


def test_updates_and_renders_queued_on_one_stream():
    import torch

    seed = uc.KEPT[1]
    hs, _ = ss.load(uc.fuzz_scenes.scene(seed, uc.W, uc.H))
    posA = hs.soa_arrays()["vertex_pos"].copy()
    posB = uc.pos_b(seed)
    posC = 0.5 * (posA + posB)
    dev = rtamd.DeviceScene(hs, 0)
    p = _params(hs)
    outs = [torch.zeros((uc.H, uc.W, 3), dtype=torch.float64, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for pos, out in zip((posB, posC), outs):   # no host synchronisation in between
        hs.update_vertices(pos)
        dev.update(hs, stream=stream.cuda_stream)
        dev.launch(p, out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    got = [o.cpu().numpy() for o in outs]
    want = []
    for pos in (posB, posC):
        hs.update_vertices(pos)
        fresh = rtamd.DeviceScene(hs, 0)
        want.append(fresh.render(p)[0])
        fresh.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(want[0], want[1])
    dev.close()
