"""Occlusion fans generated on the device (DeviceScene.ao: rt_trace_ao).  The reference
is k minus the per-point sum of DeviceScene.trace(ao_rays_host(...), occluded=True) -- the fan rays
written out by the host function and decided by the entry point test_query_gpu.py pins to the
oracle.  Counts are integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
import rtamd
from rtamd import abi

import ao_cases
import fuzz_scenes
import kat_scenes
import query_cases as qc

pytestmark = pytest.mark.gpu

SPILL_SCENE = ("random_tris", 20000, "reference")   # test_query_gpu.py's
GUARD = 0x5a5a5a5a

_dev, _pts = {}, {}


def _scene(name):
    return qc.scene(name, qc.SCENES[name].get("n_triangles", 0))


def _device(name, tree):
    """One upload per (scene, tree), shared by the tests of this module."""
    if (name, tree) not in _dev:
        _dev[(name, tree)] = rtamd.DeviceScene(_scene(name)[0], 0, tree=tree)
    return _dev[(name, tree)]


def _camera_points(hs, dev):
    """The hit points of a 32 x 24 camera as point records (numpy): 768, misses degenerate."""
    import torch

    rays = torch.from_numpy(rtamd.camera_rays(hs.render_params(32, 24, 1))).cuda()
    pts = rtamd.ao_points_from_hits(rays, dev.trace(rays)).cpu().numpy()
    assert pts.shape == (768, 8)
    return pts


def _points(name, tree):
    if (name, tree) not in _pts:
        _pts[(name, tree)] = _camera_points(_scene(name)[0], _device(name, tree))
    return _pts[(name, tree)]


def _half_diagonal(dev):
    lo, hi = dev.bounds()
    e = hi - lo
    return 0.5 * np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])


def _office_points():
    """The office's points with half the root box's diagonal as radius: the room is closed, so only
    a bounded fan is partly open there."""
    pts = _points("office", None).copy()
    pts[:, 6] = _half_diagonal(_device("office", None))
    return pts


def _reference(dev, pts, dirs, seed, bias):
    """(unoccluded counts, occluded rays) from the materialised fan through rt_trace_occluded."""
    k = dirs.shape[1]
    occ = dev.trace(rtamd.ao_rays_host(pts, dirs, seed, bias), occluded=True)
    assert set(np.unique(occ)) <= {0, 1}
    occ = occ.reshape(len(pts), k).astype(np.int64)
    return k - occ.sum(axis=1), int(occ.sum())


def _check(dev, pts, dirs, seed=0, bias=0.0):
    """ao() against the reference: counts, stats.rays and stats.hits, exactly.  Returns the counts."""
    want, hits = _reference(dev, pts, dirs, seed, bias)
    got, st = dev.ao(pts, dirs, seed=seed, bias=bias, stats=True)
    assert got.dtype == np.int32 and got.shape == (len(pts),)
    print(f"n {len(pts)} k {dirs.shape[1]}: counts min {want.min()} max {want.max()}, occluded {hits}, "
          f"differing points {int((got != want).sum())}, spills {st.stack_spills}")
    assert np.array_equal(got, want)
    assert st.rays == len(pts) * dirs.shape[1] and st.hits == hits and st.watchdog == 0
    assert dev.status() == abi.RT_OK
    return want


@pytest.mark.parametrize("radius", ["inf", "half_diagonal"])
@pytest.mark.parametrize("name,tree", [("cornell", None), ("office", None), ("random_tris", "reference")])
def test_scenes(gpu_available, name, tree, radius):
    dev = _device(name, tree)
    pts = _points(name, tree).copy()
    k = 16
    if radius != "inf":   # half the root box's diagonal: some fan rays are blocked and some are not
        pts[:, 6] = _half_diagonal(dev)
    dirs = rtamd.ao_directions(k, 7, seed=1)
    want = _check(dev, pts, dirs, seed=3, bias=1e-6)
    # the comparison cannot pass on all-equal data: the reference holds partly open fans
    if name == "office" and radius == "inf":
        # the office is a closed room and the camera sees no background: every unbounded fan ray is
        # blocked, so this case pins the all-occluded extreme and the finite radius the mixed one
        assert np.all(want == 0)
    else:
        assert np.any((want > 0) & (want < k))
    if name == "cornell":
        assert np.any(want == 0) and np.any(want == k)


@pytest.mark.parametrize("k", [1, 3, 16, 63, 64, 65, 100])
def test_sample_counts(gpu_available, k):
    # runs of k lanes that start mid-wave, span waves and span blocks
    dev = _device("cornell", None)
    want = _check(dev, _points("cornell", None), rtamd.ao_directions(k, 5, seed=k), seed=k, bias=1e-6)
    assert want.min() < want.max()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_point_counts(gpu_available, n):
    import torch

    dev = _device("cornell", None)
    pts = _points("cornell", None)
    sub = np.ascontiguousarray(pts[100:100 + n])   # image row 3 onwards: hits and misses
    dirs = rtamd.ao_directions(5, 3, seed=2)
    want, hits = _reference(dev, sub, dirs, 9, 1e-6)
    d_pts = torch.from_numpy(pts[100:]).cuda()   # more points behind the n-th: not to be read as results
    d_dirs = torch.from_numpy(dirs).cuda()
    out = torch.full((n + 64,), GUARD, dtype=torch.int32, device="cuda")
    a = abi.AoParams(k=5, n_sets=3, seed=9, bias=1e-6, d_dirs=d_dirs.data_ptr())
    st = abi.QueryStats()
    rc = rtamd.hip_lib().rt_trace_ao(dev._h, d_pts.data_ptr(), n, C.byref(a), out.data_ptr(), C.byref(st), None)
    assert rc == abi.RT_OK, rtamd.hip_lib().rt_last_error()
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], want) and np.all(got[n:] == GUARD)
    assert (st.rays, st.hits) == (5 * n, hits)


def test_zero_points_touch_nothing(gpu_available):
    import torch

    dev = _device("cornell", None)
    lib = rtamd.hip_lib()
    d_pts = torch.from_numpy(_points("cornell", None)[:4].copy()).cuda()
    d_dirs = torch.from_numpy(rtamd.ao_directions(5, 3)).cuda()
    out = torch.full((4,), GUARD, dtype=torch.int32, device="cuda")
    a = abi.AoParams(k=5, n_sets=3, seed=0, bias=0.0, d_dirs=d_dirs.data_ptr())
    st = abi.QueryStats(rays=-1)
    assert lib.rt_trace_ao(dev._h, d_pts.data_ptr(), 0, C.byref(a), out.data_ptr(), C.byref(st), None) == abi.RT_OK
    assert (st.rays, st.hits) == (0, 0)
    assert lib.rt_trace_ao(dev._h, None, 0, C.byref(a), None, None, None) == abi.RT_OK
    torch.cuda.synchronize()
    assert bool((out == GUARD).all())
    got = dev.ao(np.zeros((0, 8)), rtamd.ao_directions(5, 3))
    assert got.shape == (0,) and got.dtype == np.int32


def test_parameters(gpu_available):
    dev = _device("office", None)
    pts = _office_points()
    dirs = rtamd.ao_directions(16, 7, seed=4)
    for bias in (0.0, 1e-3):
        _check(dev, pts, dirs, seed=1, bias=bias)
    _check(dev, pts, dirs[:1], seed=1, bias=1e-6)   # n_sets = 1
    # two seeds: different set choices, each equal to its own reference
    assert not np.array_equal(ao_cases.numpy_sets(len(pts), 1, 7), ao_cases.numpy_sets(len(pts), 2, 7))
    a = _check(dev, pts, dirs, seed=1, bias=1e-6)
    b = _check(dev, pts, dirs, seed=2, bias=1e-6)
    assert not np.array_equal(a, b)


def test_degenerate_points(gpu_available):
    dev = _device("cornell", None)
    pts = _points("cornell", None)
    valid = pts[ao_cases.numpy_valid(pts)][:300]
    assert len(valid) == 300
    bad = ao_cases.degenerate_points()
    k = 9
    dirs = rtamd.ao_directions(k, 1, seed=6)   # one set: a point's fan does not depend on its index
    alone = _check(dev, valid, dirs, bias=1e-6)
    assert alone.min() < k
    # the degenerate points spread among the valid ones
    at = np.arange(len(bad)) * 23 + 5
    mixed = np.insert(valid, at - np.arange(len(bad)), bad, axis=0)
    assert ao_cases.same_bits(mixed[at], bad)
    got = _check(dev, mixed, dirs, bias=1e-6)
    keep = np.ones(len(mixed), bool)
    keep[at] = False
    assert np.all(got[at] == k) and np.array_equal(got[keep], alone)


def test_analytic_primitives(gpu_available, tmp_path):
    hs = rtamd.HostScene.load(fuzz_scenes.write_analytic(tmp_path, 3, 64, 48))
    hs.prepare()
    assert hs.raw.contents.n_spheres >= 1
    dev = rtamd.DeviceScene(hs, 0, analytic=True)
    plain = rtamd.DeviceScene(hs, 0)
    pts = _camera_points(hs, dev)
    dirs = rtamd.ao_directions(16, 7, seed=8)
    want = _check(dev, pts, dirs, seed=5, bias=1e-6)
    # the primitives take part: without them other rays are blocked
    assert not np.array_equal(want, _reference(plain, pts, dirs, 5, 1e-6)[0])
    dev.close()
    plain.close()


def test_stack_spill_path(gpu_available):
    name, n_tri, tree = SPILL_SCENE
    assert qc.SCENES[name]["n_triangles"] == n_tri
    dev = _device(name, tree)
    pts = _points(name, tree)
    dirs = rtamd.ao_directions(16, 7, seed=9)
    want, hits = _reference(dev, pts, dirs, 0, 0.0)
    got, st = dev.ao(pts, dirs, stats=True)
    print(f"spill scene: stack_spills {st.stack_spills}, occluded {hits} of {st.rays}")
    assert st.stack_spills > 0   # without it this test proves nothing about the spill path
    assert np.array_equal(got, want) and st.hits == hits
    assert np.any((want > 0) & (want < 16))


def test_one_triangle_against_the_oracle(gpu_available, tmp_path):
    # without rt_trace_occluded: the oracle's closest hit of every fan ray, t < tmax
    hs = rtamd.HostScene.load(kat_scenes.write(tmp_path, "one_tri"))
    hs.prepare()
    orc = pyoracle.Oracle(hs.raw, hs)
    gx, gy = np.meshgrid(np.linspace(-1.6, 1.6, 8), np.linspace(-1.4, 1.4, 8))
    p = np.stack([gx.ravel(), gy.ravel(), np.full(64, 2.0)], 1)
    tmax = np.where(np.arange(64) % 4 == 0, 1.5, np.where(np.arange(64) % 4 == 1, 2.5, np.inf))
    pts = ao_cases.make_points(p, np.tile([0.1, -0.2, -3.0], (64, 1)), tmax)   # facing the triangle, not unit
    k = 8
    dirs = rtamd.ao_directions(k, 3, seed=12)
    rays = rtamd.ao_rays_host(pts, dirs, 7, 1e-3)
    occ = np.zeros(len(rays), np.int64)
    for i, r in enumerate(rays):
        h = orc.closest_hit(r[0:3], r[3:6], pyoracle.MODE_REFERENCE)
        occ[i] = h is not None and h["t"] < r[6]
    want = k - occ.reshape(64, k).sum(1)
    assert np.any(want == k) and np.any(want < k)
    assert np.all(want[0::4] == k)   # the triangle is farther than tmax = 1.5
    dev = rtamd.DeviceScene(hs, 0)
    got, st = dev.ao(pts, dirs, seed=7, bias=1e-3, stats=True)
    assert np.array_equal(got, want) and st.hits == int(occ.sum()) and st.rays == 64 * k
    dev.close()


def test_ao_beside_a_render_on_another_stream(gpu_available):
    import torch

    hs = _scene("office")[0]
    dev = _device("office", None)
    pts = torch.from_numpy(_office_points()).cuda()
    dirs = torch.from_numpy(rtamd.ao_directions(65, 7, seed=3)).cuda()
    p = hs.render_params(96, 54, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    solo = dev.ao(pts, dirs, seed=1, bias=1e-6).clone()
    serial = torch.zeros((20, 54, 96, 3), dtype=torch.float64, device="cuda")
    dev.launch_frames(p, [serial[f].data_ptr() for f in range(20)])
    torch.cuda.synchronize()
    frames = torch.zeros_like(serial)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dev.launch_frames(p, [frames[f].data_ptr() for f in range(20)], stream=s1.cuda_stream)
    got = dev.ao(pts, dirs, seed=1, bias=1e-6, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and bool((got == solo).all())
    assert bool((frames == serial).all())
    assert int(solo.min()) < int(solo.max())
    assert dev.status() == abi.RT_OK


@pytest.mark.parametrize("k", [16, 65])
def test_repeatable(gpu_available, k):
    # k = 65 sums with atomics: integer, so still identical
    import torch

    dev = _device("office", None)
    pts = torch.from_numpy(_office_points()).cuda()
    dirs = torch.from_numpy(rtamd.ao_directions(k, 7, seed=3)).cuda()
    a = dev.ao(pts, dirs, seed=1, bias=1e-6).clone()
    b = dev.ao(pts, dirs, seed=1, bias=1e-6)
    assert bool((a == b).all()) and int(a.min()) < int(a.max())


def test_python_layer_checks_its_inputs(gpu_available):
    import torch

    dev = _device("cornell", None)
    with pytest.raises(ValueError):
        dev.ao(np.zeros((4, 7)), np.zeros((1, 1, 3)))
    with pytest.raises(ValueError):
        dev.ao(torch.zeros((4, 8), dtype=torch.float32, device="cuda"), np.zeros((1, 1, 3)))
    with pytest.raises(ValueError):
        dev.ao(np.zeros((4, 8)), torch.zeros((1, 1, 3), dtype=torch.float64))   # dirs not on the device
    with pytest.raises(rtamd.RtError):
        dev.ao(np.zeros((4, 8)), np.zeros((1, abi.RT_AO_MAX_SAMPLES + 1, 3)))
