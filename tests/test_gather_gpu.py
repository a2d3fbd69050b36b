"""DeviceScene.gather (rt_trace_gather) on the MI355X: the mean radiance of fans built
on the device.  The reference is the written-out computation the header defines it by:

    R = dev.radiance(rtamd.ao_rays_host(points, dirs, seed, bias), params in fp64)
    want[i] = (((0 + R[i k]) + R[i k + 1]) + ... + R[i k + k - 1]) / k

summed by an explicit loop over the samples (np.sum is pairwise).  fp64 results are compared with
np.array_equal, fp32 results with want.astype(float32), ray counts exactly."""
import ctypes as C

import numpy as np
import pytest

import rtamd
from rtamd import abi

import ao_cases
import radiance_cases as rc

pytestmark = pytest.mark.gpu

GUARD = -7.0

_dev, _pts = {}, {}


def _device(name, tree=None, ring=8):
    """One upload per (scene, tree, stack ring), shared by the tests of this module."""
    key = (name, tree, ring)
    if key not in _dev:
        _dev[key] = rtamd.DeviceScene(rc.scene(name)[0], 0, tree=tree, stack_ring=ring)
    return _dev[key]


def _camera_points(hs, dev):
    """The hit points of a 32 x 24 camera as point records (numpy): 768, misses degenerate."""
    import torch

    rays = torch.from_numpy(rtamd.camera_rays(hs.render_params(32, 24, 1))).cuda()
    pts = rtamd.ao_points_from_hits(rays, dev.trace(rays)).cpu().numpy()
    assert pts.shape == (768, 8)
    return pts


def _points(name, tree=None):
    if (name, tree) not in _pts:
        _pts[(name, tree)] = _camera_points(rc.scene(name)[0], _device(name, tree))
    return _pts[(name, tree)]


def _half_diagonal(dev):
    lo, hi = dev.bounds()
    e = hi - lo
    return 0.5 * np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])


def _params(name, **fields):
    return rc.copy_params(rc.params(rc.scene(name)[0], 8, 8), **fields)


def _reference(dev, pts, dirs, p, seed=0, bias=0.0):
    """(mean colours [n, 3], the samples [n, k, 3], Stats) of the written-out fan through radiance()."""
    n, k = len(pts), dirs.shape[1]
    R, st = dev.radiance(rtamd.ao_rays_host(pts, dirs, seed, bias), rc.copy_params(p, out_format=rtamd.RT_OUT_RGB_F64),
                         stats=True)
    R = R.reshape(n, k, 3)
    acc = np.zeros((n, 3))
    for s in range(k):   # in sample order, one add per sample
        acc = acc + R[:, s, :]
    return acc / k, R, st


def _check(dev, pts, dirs, p, seed=0, bias=0.0):
    """gather() against the reference in fp64 and fp32, ray counts exactly.  Returns (want, samples, Stats)."""
    want, R, rst = _reference(dev, pts, dirs, p, seed, bias)
    got, st = dev.gather(pts, dirs, rc.copy_params(p, out_format=rtamd.RT_OUT_RGB_F64), seed=seed, bias=bias, stats=True)
    assert got.dtype == np.float64 and got.shape == (len(pts), 3)
    diff = got != want
    print(f"n {len(pts)} k {dirs.shape[1]}: differing values {int(diff.sum())}, max |diff| "
          f"{float(np.abs(got - want).max()) if len(pts) else 0.0:.3e}, rays P/S/R {rc.counts(st)} (reference {rc.counts(rst)})")
    assert np.array_equal(got, want)
    assert rc.counts(st) == rc.counts(rst)
    assert st.pixels == len(pts) and st.node_visits == 0 and st.tri_tests == 0 and st.closest_hits == 0
    got32 = dev.gather(pts, dirs, rc.copy_params(p, out_format=rtamd.RT_OUT_RGB_F32), seed=seed, bias=bias)
    assert got32.dtype == np.float32 and np.array_equal(got32, want.astype(np.float32))
    assert dev.status() == abi.RT_OK
    return want, R, st


def _not_trivial(want, R):
    """At least two points with different colours and one point whose samples are not all equal."""
    assert len(np.unique(want, axis=0)) >= 2
    assert np.any(np.any(R != R[:, :1, :], axis=(1, 2)))


# ---- 1. scenes, radii, rings, depths ----
# (random_tris on the reference tree: the scene of tests/test_query_gpu.py that spills the 8-entry ring)
@pytest.mark.parametrize("own_depth", [False, True])
@pytest.mark.parametrize("ring", [8, 16])
@pytest.mark.parametrize("radius", ["inf", "half_diagonal"])
@pytest.mark.parametrize("name,tree", [("cornell", None), ("office", None), ("random_tris", "reference")])
def test_scenes(gpu_available, name, tree, radius, ring, own_depth):
    dev = _device(name, tree, ring)
    pts = _points(name, tree).copy()
    if radius != "inf":
        pts[:, 6] = _half_diagonal(dev)
    p = _params(name)
    if not own_depth:
        p.max_depth = 0
    want, R, st = _check(dev, pts, rtamd.ao_directions(16, 7, seed=1), p, seed=3, bias=1e-6)
    _not_trivial(want, R)
    assert st.primary_rays > 0
    if name == "office" and own_depth:
        assert p.max_depth > 0 and st.reflection_rays > 0
    if not own_depth:
        assert st.reflection_rays == 0


# ---- 2. group sizes: G = 1, partial last chunks at G = 2 and G = 32, four chunks ----
@pytest.mark.parametrize("k", [1, 2, 3, 16, 31, 32, 33, 64, 100])
def test_sample_counts(gpu_available, k):
    dev = _device("cornell")
    want, R, _ = _check(dev, _points("cornell"), rtamd.ao_directions(k, 5, seed=k), _params("cornell"), seed=k, bias=1e-6)
    assert len(np.unique(want, axis=0)) >= 2


# ---- 3. point counts and the rows behind the result ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_point_counts(gpu_available, n):
    import torch

    dev = _device("cornell")
    pts = _points("cornell")
    sub = np.ascontiguousarray(pts[100:100 + n])   # image row 3 onwards: hits and misses
    dirs = rtamd.ao_directions(5, 3, seed=2)
    p = _params("cornell")
    want, R, rst = _reference(dev, sub, dirs, p, 9, 1e-6)
    d_pts = torch.from_numpy(pts[100:]).cuda()   # more points behind the n-th: not to be read as work
    d_dirs = torch.from_numpy(dirs).cuda()
    out = torch.full((n + 64, 3), GUARD, dtype=torch.float64, device="cuda")
    a = abi.AoParams(k=5, n_sets=3, seed=9, bias=1e-6, d_dirs=d_dirs.data_ptr())
    st = abi.Stats()
    rc_ = rtamd.hip_lib().rt_trace_gather(dev._h, C.byref(p), d_pts.data_ptr(), n, C.byref(a), out.data_ptr(),
                                          C.byref(st), None)
    assert rc_ == abi.RT_OK, rtamd.hip_lib().rt_last_error()
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], want) and np.all(got[n:] == GUARD)
    assert rc.counts(st) == rc.counts(rst) and st.pixels == n


def test_zero_points_launch_nothing_and_touch_nothing(gpu_available):
    import torch

    dev = _device("cornell")
    lib = rtamd.hip_lib()
    p = _params("cornell")
    dev.render(p)
    grid = dev.last_grid()
    d_pts = torch.from_numpy(_points("cornell")[:4].copy()).cuda()
    d_dirs = torch.from_numpy(rtamd.ao_directions(5, 3)).cuda()
    out = torch.full((4, 3), GUARD, dtype=torch.float64, device="cuda")
    a = abi.AoParams(k=5, n_sets=3, seed=0, bias=0.0, d_dirs=d_dirs.data_ptr())
    st = abi.Stats(primary_rays=-1, pixels=-1)
    assert lib.rt_trace_gather(dev._h, C.byref(p), d_pts.data_ptr(), 0, C.byref(a), out.data_ptr(), C.byref(st),
                               None) == abi.RT_OK
    assert lib.rt_trace_gather(dev._h, C.byref(p), None, 0, C.byref(a), None, None, None) == abi.RT_OK
    torch.cuda.synchronize()
    assert bool((out == GUARD).all())
    assert (st.primary_rays, st.pixels) == (0, 0)
    assert dev.last_grid() == grid   # no launch was recorded
    got = dev.gather(np.zeros((0, 8)), rtamd.ao_directions(5, 3), p)
    assert got.shape == (0, 3) and got.dtype == np.float64


# ---- 4. the clamp is per sample ----
def test_samples_are_clamped_before_they_are_added(gpu_available):
    dev = _device("cornell")
    p = _params("cornell")
    for i in range(p.n_lights):
        for c in range(3):
            p.lights[i].color[c] = 4.0 * p.lights[i].color[c]
    want, R, _ = _check(dev, _points("cornell"), rtamd.ao_directions(16, 7, seed=4), p, seed=5, bias=1e-6)
    # some point has, in one channel, samples at exactly 1 (clamped) and samples below 1: the mean of
    # the clamped samples then differs from the clamped mean of the unclamped ones
    at_one, below = (R == 1.0).any(axis=1), (R < 1.0).any(axis=1)
    assert np.any(at_one & below)


# ---- 5. degenerate points and directions ----
def test_degenerate_points_and_directions(gpu_available):
    dev = _device("cornell")
    pts = _points("cornell")
    valid = pts[ao_cases.numpy_valid(pts)][:300]
    assert len(valid) == 300
    bad = ao_cases.degenerate_points()   # NaN / inf o, NaN / inf / zero / underflowing normal, NaN tmax, tmax <= 1e-5
    k = 9
    dirs = rtamd.ao_directions(k, 1, seed=6)   # one set: a point's fan does not depend on its index
    dirs[:, 2] = [0.0, 0.0, 0.0]
    dirs[:, 5] = [np.nan, 0.0, 1.0]
    p = _params("cornell")
    alone, R, st0 = _check(dev, valid, dirs, p, bias=1e-6)
    # the two degenerate directions take the background and are not counted
    bg = rc.background(p)
    assert np.all(R[:, 2] == bg) and np.all(R[:, 5] == bg) and st0.primary_rays == len(valid) * (k - 2)
    at = np.arange(len(bad)) * 23 + 5   # the degenerate points spread among the valid ones
    mixed = np.insert(valid, at - np.arange(len(bad)), bad, axis=0)
    assert ao_cases.same_bits(mixed[at], bad)
    got, _, st = _check(dev, mixed, dirs, p, bias=1e-6)
    keep = np.ones(len(mixed), bool)
    keep[at] = False
    assert np.array_equal(got[keep], alone) and rc.counts(st) == rc.counts(st0)
    # a fully degenerate point: k times min(background, 1), summed in order and divided
    acc = np.zeros(3)
    for _ in range(k):
        acc = acc + bg
    assert np.all(got[at] == acc / k)
    only_bad, _, sb = _check(dev, bad, dirs, p)   # a launch that never traverses
    assert np.all(only_bad == acc / k) and rc.counts(sb) == [0, 0, 0]


# ---- 6. analytic primitives, lights ----
def test_analytic_primitives(gpu_available):
    hs = rtamd.HostScene.generate("spheres")
    hs.prepare()
    dev = rtamd.DeviceScene(hs, 0, analytic=True)
    pts = _camera_points(hs, dev)
    p = rc.params(hs, 8, 8)
    want, R, st = _check(dev, pts, rtamd.ao_directions(16, 7, seed=8), p, seed=5, bias=1e-6)
    _not_trivial(want, R)
    assert st.shadow_rays > 0 and st.reflection_rays > 0
    dev.close()


def test_seventeen_lights_then_two(gpu_available):
    dev = _device("cornell")
    pts = _points("cornell")
    p2 = _params("cornell")
    assert p2.n_lights >= 2
    p2.n_lights = 2
    base = [(tuple(p2.lights[i].position), tuple(p2.lights[i].color)) for i in range(2)]
    p17 = _params("cornell")
    lights = []
    for i in range(17):
        a = 2.0 * np.pi * i / 17
        pos, _ = base[i % 2]
        lights.append(((pos[0] + 0.3 * np.cos(a), pos[1], pos[2] + 0.3 * np.sin(a)), (0.1 + 0.02 * (i % 5),) * 3))
    p17.set_lights(lights)
    assert p17.n_lights == 17 and bool(p17.lights_ext)
    dirs = rtamd.ao_directions(16, 7, seed=2)
    seen = []
    for p in (p17, p2):   # the light table is copied with every launch: 2 lights after 17
        want, R, st = _check(dev, pts, dirs, p, seed=1, bias=1e-6)
        _not_trivial(want, R)
        seen.append((want, st.shadow_rays))
    assert not np.array_equal(seen[0][0], seen[1][0]) and seen[0][1] > seen[1][1]


# ---- 7. fan parameters ----
def test_fan_parameters(gpu_available):
    dev = _device("office")
    pts = _points("office").copy()
    pts[:, 6] = _half_diagonal(dev)
    p = _params("office")
    dirs = rtamd.ao_directions(16, 7, seed=4)
    b0 = _check(dev, pts, dirs, p, seed=1, bias=0.0)[0]
    b3 = _check(dev, pts, dirs, p, seed=1, bias=1e-3)[0]
    assert not np.array_equal(b0, b3)
    _check(dev, pts, dirs[:1], p, seed=1, bias=1e-6)   # n_sets = 1
    # two seeds: different set choices, each equal to its own reference
    assert not np.array_equal(ao_cases.numpy_sets(len(pts), 1, 7), ao_cases.numpy_sets(len(pts), 2, 7))
    a = _check(dev, pts, dirs, p, seed=1, bias=1e-6)[0]
    b = _check(dev, pts, dirs, p, seed=2, bias=1e-6)[0]
    assert not np.array_equal(a, b)


# ---- 8. straight against the oracle ----
def test_sixty_four_points_against_the_oracle(gpu_available):
    hs, orc = rc.scene("cornell")
    dev = _device("cornell")
    pts = _points("cornell")
    pts = np.ascontiguousarray(pts[ao_cases.numpy_valid(pts)][::7][:64])
    assert len(pts) == 64
    k = 8
    dirs = rtamd.ao_directions(k, 3, seed=12)
    p = _params("cornell")
    rays = rtamd.ao_rays_host(pts, dirs, 7, 1e-6)
    # each fan ray as the one pixel of a 1 x 1 oracle camera: eye = the ray's origin, lower_left =
    # origin + 1024 d (the oracle subtracts the eye again; the factor keeps that round trip's error
    # far below the direction's last bit times the scene's size)
    o = rays[:, 0:3]
    col, cnt = rc.oracle_single_rays(("cornell", "gather", k), orc, p, o, o + 1024.0 * rays[:, 3:6])
    col = np.minimum(col, 1.0).reshape(64, k, 3)
    want = np.zeros((64, 3))
    for s in range(k):
        want = want + col[:, s, :]
    want = want / k
    got, st = dev.gather(pts, dirs, p, seed=7, bias=1e-6, stats=True)
    err = float(np.abs(got - want).max())
    print(f"gather against the oracle: max |diff| {err:.3e}, rays P/S/R {rc.counts(st)} (oracle {cnt})")
    assert err <= rc.TOL64
    assert len(np.unique(want, axis=0)) >= 2


# ---- 9. beside and between renders ----
def test_gather_beside_a_render_on_another_stream(gpu_available):
    import torch

    hs, _ = rc.scene("office")
    dev = _device("office")
    p = _params("office")
    pts = _points("office").copy()
    pts[:, 6] = _half_diagonal(dev)
    d_pts = torch.from_numpy(pts).cuda()
    d_dirs = torch.from_numpy(rtamd.ao_directions(33, 7, seed=3)).cuda()
    pf = rc.params(hs, 96, 54)
    solo = dev.gather(d_pts, d_dirs, p, seed=1, bias=1e-6).clone()
    serial = torch.zeros((20, 54, 96, 3), dtype=torch.float64, device="cuda")
    dev.launch_frames(pf, [serial[f].data_ptr() for f in range(20)])
    torch.cuda.synchronize()
    frames = torch.zeros_like(serial)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dev.launch_frames(pf, [frames[f].data_ptr() for f in range(20)], stream=s1.cuda_stream)
    got = dev.gather(d_pts, d_dirs, p, seed=1, bias=1e-6, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and bool((got == solo).all())
    assert bool((frames == serial).all())
    assert len(torch.unique(solo, dim=0)) >= 2
    assert dev.status() == abi.RT_OK


def test_frame_launches_behave_as_if_the_gather_call_had_not_happened(gpu_available):
    """As the radiance test of the same name: two one-frame launches, a gather call, a third launch
    -- three identical images, and the cost-order sequence goes on as on a control scene that gets
    no gather call."""
    hs, _ = rc.scene("cornell")
    lib = rtamd.hip_lib()
    W, H = 64, 48
    p = rc.params(hs, W, H)
    tw, th = rtamd.tile_shape()
    n_tiles = -(-W // tw) * -(-H // th)
    pts = _points("cornell")
    dirs = rtamd.ao_directions(16, 7, seed=1)
    want = _reference(_device("cornell"), pts, dirs, p, 3, 1e-6)[0]

    def order_len(dev):
        return int(lib.rt_debug_last_tile_order(dev._h, None, 0))

    seen = {}
    for with_gather in (False, True):
        dev = rtamd.DeviceScene(hs, 0)
        a, _ = dev.render(p)
        b, _ = dev.render(p)
        m2 = order_len(dev)
        if with_gather:
            assert np.array_equal(dev.gather(pts, dirs, p, seed=3, bias=1e-6), want)
            assert order_len(dev) == m2
        c, _ = dev.render(p)
        m3 = order_len(dev)
        assert np.array_equal(a, b) and np.array_equal(a, c)
        got = np.zeros(max(1, m3), dtype=np.uint32)
        lib.rt_debug_last_tile_order(dev._h, got.ctypes.data_as(C.POINTER(C.c_uint)), m3)
        assert m3 == n_tiles and np.array_equal(np.sort(got[:m3]), np.arange(n_tiles))
        seen[with_gather] = (m2, m3)
        dev.close()
    assert seen[True] == seen[False]


# ---- 10. repeatability ----
@pytest.mark.parametrize("k", [16, 33])
def test_repeatable(gpu_available, k):
    import torch

    dev = _device("office")
    pts = _points("office").copy()
    pts[:, 6] = _half_diagonal(dev)
    d_pts = torch.from_numpy(pts).cuda()
    d_dirs = torch.from_numpy(rtamd.ao_directions(k, 7, seed=3)).cuda()
    p = _params("office")
    a = dev.gather(d_pts, d_dirs, p, seed=1, bias=1e-6).clone()
    b = dev.gather(d_pts, d_dirs, p, seed=1, bias=1e-6)
    assert bool((a == b).all()) and len(torch.unique(a, dim=0)) >= 2


def test_diagnostics_know_the_new_kernels(gpu_available):
    dev = _device("cornell")
    lib = rtamd.hip_lib()
    for v in (9, 10):
        assert 1 <= lib.rt_debug_blocks_per_cu(dev._h, v) <= 4
    assert lib.rt_debug_blocks_per_cu(dev._h, 11) == abi.RT_ERR_INVALID
