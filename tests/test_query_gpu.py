"""Batched ray queries (DeviceScene.trace: rt_trace_closest / rt_trace_occluded) against the CPU
oracle.  Every comparison is exact: t, normal, alpha and beta are IEEE fp64 + - x / sqrt in the
oracle's order without contraction, so a last-bit difference is a bug."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
import rtamd
from rtamd import abi

import fuzz_scenes
import kat_scenes
import query_cases as qc

pytestmark = pytest.mark.gpu

TREES = [None, "sah", "reference"]
REF, ORD = pyoracle.MODE_REFERENCE, pyoracle.MODE_ORDERED
# the smallest generated scene whose rays (case 1's) spill the 8-entry LDS stack ring
SPILL_SCENE = ("random_tris", 20000, "reference")


def _scene(name):
    return qc.scene(name, qc.SCENES[name].get("n_triangles", 0))


_dev = {}


def _device(name, tree):
    """One upload per (scene, tree), shared by the tests of this module."""
    if (name, tree) not in _dev:
        _dev[(name, tree)] = rtamd.DeviceScene(_scene(name)[0], 0, tree=tree)
    return _dev[(name, tree)]


def _case1(name):
    hs, orc, P, vidx, perm = _scene(name)
    rays = qc.random_rays(hs)
    return rays, qc.expected((name, "random"), orc, rays, REF)


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", sorted(qc.SCENES))
def test_random_rays_match_oracle(gpu_available, name, tree):
    hs, orc, P, vidx, perm = _scene(name)
    rays, want = _case1(name)
    got, st = _device(name, tree).trace(rays, stats=True)
    qc.check_hits(got, want, rays, P, vidx, perm)
    assert st.rays == 4096 and st.hits == int(want["hit"].sum()) and st.watchdog == 0
    occ = _device(name, tree).trace(rays, occluded=True)
    assert np.array_equal(occ.astype(bool), want["hit"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partial_waves_and_blocks(gpu_available, n):
    import torch

    hs, orc, P, vidx, perm = _scene("cornell")
    rays, want = _case1("cornell")
    dev = _device("cornell", None)
    # results behind the n-th stay untouched
    d_rays = torch.from_numpy(rays).cuda()
    got, st = dev.trace(d_rays[:n].contiguous(), stats=True)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    sub = {k: v[:n] for k, v in want.items()}
    qc.check_hits(got, sub, rays[:n], P, vidx, perm)
    assert st.rays == n and st.hits == int(sub["hit"].sum())
    occ = dev.trace(rays[:n], occluded=True)
    assert occ.shape == (n,) and np.array_equal(occ.astype(bool), sub["hit"])


def test_zero_rays_touch_nothing(gpu_available):
    import torch

    dev = _device("cornell", None)
    lib = rtamd.hip_lib()
    rays = torch.zeros((4, 8), dtype=torch.float64, device="cuda")
    hits = torch.full((4, 8), 7.0, dtype=torch.float64, device="cuda")
    occ = torch.full((4,), 7, dtype=torch.uint8, device="cuda")
    st = abi.QueryStats(rays=-1)
    assert lib.rt_trace_closest(dev._h, rays.data_ptr(), 0, hits.data_ptr(), C.byref(st), None) == abi.RT_OK
    assert (st.rays, st.hits) == (0, 0)
    assert lib.rt_trace_occluded(dev._h, rays.data_ptr(), 0, occ.data_ptr(), None, None) == abi.RT_OK
    torch.cuda.synchronize()
    assert bool((hits == 7.0).all()) and bool((occ == 7).all())
    got = dev.trace(np.zeros((0, 8)))
    assert got["t"].shape == (0,) and got["normal"].shape == (0, 3)


@pytest.mark.parametrize("name", ["cornell", "office"])
def test_vertex_aimed_rays_match_ordered_oracle(gpu_available, name):
    # ties and edges: these rays meet the measure-zero divergence of the reference box test
    # (DESIGN.md §3); the ordered mode is the one the device equals.  No ray is excluded.
    hs, orc, P, vidx, perm = _scene(name)
    rays = qc.vertex_rays(hs, P)
    want = qc.expected((name, "vertex"), orc, rays, ORD)
    for tree in (None, "reference"):
        got = _device(name, tree).trace(rays)
        qc.check_hits(got, want, rays, P, vidx, perm)


def test_axis_aligned_rays_match_oracle(gpu_available):
    hs, orc, P, vidx, perm = _scene("cornell")
    rays = qc.axis_rays(hs)
    want = qc.expected(("cornell", "axis"), orc, rays, REF)
    assert want["hit"].any() and not want["hit"].all()
    got = _device("cornell", None).trace(rays)
    qc.check_hits(got, want, rays, P, vidx, perm)


def test_finite_tmax(gpu_available):
    hs, orc, P, vidx, perm = _scene("cornell")
    rays, want = _case1("cornell")
    h = want["hit"]
    dev = _device("cornell", None)
    for tmax, hits in ((0.5 * want["t"][h], False), (want["t"][h], False), (np.nextafter(want["t"][h], np.inf), True)):
        r = rays[h].copy()
        r[:, 6] = tmax
        got = dev.trace(r)
        occ = dev.trace(r, occluded=True)
        assert np.array_equal(np.isfinite(got["t"]), np.full(len(r), hits))
        assert np.array_equal(occ, np.full(len(r), 1 if hits else 0, np.uint8))
        if hits:
            sub = {k: v[h] for k, v in want.items()}
            qc.check_hits(got, sub, r, P, vidx, perm)
        else:
            assert np.all(got["slot"] == -1) and np.all(got["normal"] == 0.0)


@pytest.mark.parametrize("name", ["cornell", "office"])
def test_occlusion_rays_to_the_lights(gpu_available, name):
    hs, orc, P, vidx, perm = _scene(name)
    rays, want = _case1(name)
    raw = hs.raw.contents
    assert raw.n_lights >= 1
    pts = want["point"][want["hit"]]
    dev = _device(name, None)
    for li in range(raw.n_lights):
        l = np.array(raw.lights[li].position[:])
        d = l - pts
        tmax = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        r = qc.make_rays(pts, d, tmax)
        exp = qc.expected((name, "light", li), orc, r, REF)
        blocked = exp["hit"] & (exp["t"] < tmax)
        assert blocked.any() and not blocked.all()
        occ = dev.trace(r, occluded=True)
        assert np.array_equal(occ.astype(bool), blocked)
        got = dev.trace(r)
        assert np.array_equal(np.isfinite(got["t"]), blocked)
        assert np.array_equal(got["t"][blocked], exp["t"][blocked])


def test_degenerate_rays_are_misses(gpu_available):
    hs, orc, P, vidx, perm = _scene("cornell")
    rays, want = _case1("cornell")
    good = rays[want["hit"]][:16]
    bad = []
    for col, val in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, -np.inf),
                     (6, np.nan), (6, 0.0), (6, 1e-5), (6, -1.0)):
        r = good.copy()
        r[:, col] = val
        bad.append(r)
    z = good.copy()
    z[:, 3:6] = 0.0
    bad.append(z)
    r = np.concatenate(bad + [good])   # the good rays after them still hit
    dev = _device("cornell", None)
    got, st = dev.trace(r, stats=True)
    nb = len(r) - len(good)
    assert np.all(np.isinf(got["t"][:nb])) and np.all(got["t"][:nb] > 0)
    assert np.all(got["slot"][:nb] == -1) and np.all(got["mesh"][:nb] == -1) and np.all(got["prim"][:nb] == -1)
    assert np.all(got["normal"][:nb] == 0.0) and np.all(got["alpha"][:nb] == 0.0) and np.all(got["beta"][:nb] == 0.0)
    assert np.all(np.isfinite(got["t"][nb:]))
    assert st.hits == len(good)
    occ = dev.trace(r, occluded=True)
    assert np.array_equal(occ, np.concatenate([np.zeros(nb, np.uint8), np.ones(len(good), np.uint8)]))
    assert dev.status() == abi.RT_OK


def test_analytic_primitives(gpu_available, tmp_path):
    hs = rtamd.HostScene.load(fuzz_scenes.write_analytic(tmp_path, 3, 64, 48))
    hs.prepare()
    raw = hs.raw.contents
    n_prims = raw.n_spheres + raw.n_planes
    assert raw.n_spheres >= 1
    orc = pyoracle.Oracle(hs.raw, hs)
    soa = hs.soa_arrays()
    P, vidx, perm = soa["vertex_pos"], soa["vertex_idx"], orc.bvh()["perm"]
    rays = qc.random_rays(hs, 1024)
    want = qc.oracle_hits(orc, rays, REF)
    alt = qc.oracle_hits(orc, rays, ORD)
    differ = (want["hit"] != alt["hit"]) | (want["t"] != alt["t"]) | (want["tri"] != alt["tri"])
    assert differ.sum() <= len(rays) // 100
    assert (want["tri"][want["hit"]] == -1).any()   # analytic hits are in the set
    dev = rtamd.DeviceScene(hs, 0, analytic=True)
    got = dev.trace(rays)
    qc.check_hits(got, want, rays, P, vidx, perm, analytic=True, only=~differ)
    if differ.any():
        qc.check_hits(got, alt, rays, P, vidx, perm, analytic=True, only=differ)
    prim = got["prim"][np.isfinite(got["t"]) & (got["slot"] == -1)]
    assert np.all((prim >= 0) & (prim < n_prims))
    occ = dev.trace(rays, occluded=True)
    assert np.array_equal(occ.astype(bool), want["hit"])
    dev.close()


def test_single_leaf_root(gpu_available, tmp_path):
    # one triangle: the root's sibling slots are empty (kEmpty)
    hs = rtamd.HostScene.load(kat_scenes.write(tmp_path, "one_tri"))
    hs.prepare()
    orc = pyoracle.Oracle(hs.raw, hs)
    soa = hs.soa_arrays()
    gx, gy = np.meshgrid(np.linspace(-1.6, 1.6, 8), np.linspace(-1.4, 1.4, 8))
    target = np.stack([gx.ravel(), gy.ravel(), np.zeros(64)], 1)
    o = np.tile(np.array([0.3, -0.2, 4.0]), (64, 1))
    rays = qc.make_rays(o, target - o)
    want = qc.oracle_hits(orc, rays, REF)
    assert want["hit"].any() and not want["hit"].all()
    for tree in TREES:
        dev = rtamd.DeviceScene(hs, 0, tree=tree)
        got = dev.trace(rays)
        qc.check_hits(got, want, rays, soa["vertex_pos"], soa["vertex_idx"], orc.bvh()["perm"])
        assert np.array_equal(dev.trace(rays, occluded=True).astype(bool), want["hit"])
        dev.close()


def test_stack_spill_path(gpu_available):
    name, n_tri, tree = SPILL_SCENE
    assert qc.SCENES[name]["n_triangles"] == n_tri
    hs, orc, P, vidx, perm = _scene(name)
    rays, want = _case1(name)
    dev = _device(name, tree)
    got, st = dev.trace(rays, stats=True)
    assert st.stack_spills > 0   # without it this test proves nothing about the spill path
    qc.check_hits(got, want, rays, P, vidx, perm)
    occ, so = dev.trace(rays, occluded=True, stats=True)
    assert np.array_equal(occ.astype(bool), want["hit"]) and so.hits == int(want["hit"].sum())


def test_primary_hits_equal_the_render_kernels(gpu_available):
    hs, orc, P, vidx, perm = _scene("office")
    dev = _device("office", None)
    p = hs.render_params(96, 54, 1)
    p.max_depth = 0
    p.flags = rtamd.RT_FLAG_TRAVERSAL_STATS
    _, rst = dev.render(p)
    got, st = dev.trace(rtamd.camera_rays(p), stats=True)
    assert st.rays == 96 * 54
    assert st.hits == rst.closest_hits == int(np.isfinite(got["t"]).sum())


def test_query_beside_a_render_on_another_stream(gpu_available):
    import torch

    hs, orc, P, vidx, perm = _scene("office")
    dev = _device("office", None)
    rays = torch.from_numpy(qc.random_rays(hs)).cuda()
    p = hs.render_params(96, 54, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    serial_hits = {k: v.clone() for k, v in dev.trace(rays).items()}
    serial = torch.zeros((20, 54, 96, 3), dtype=torch.float64, device="cuda")
    dev.launch_frames(p, [serial[f].data_ptr() for f in range(20)])
    torch.cuda.synchronize()
    frames = torch.zeros_like(serial)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dev.launch_frames(p, [frames[f].data_ptr() for f in range(20)], stream=s1.cuda_stream)
    got = dev.trace(rays, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    for k, v in serial_hits.items():
        a, b = v.cpu().numpy(), got[k].cpu().numpy()
        assert np.array_equal(a, b, equal_nan=False), k
    assert bool((frames == serial).all())
    assert dev.status() == abi.RT_OK
