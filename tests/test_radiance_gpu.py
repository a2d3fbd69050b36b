"""DeviceScene.radiance (rt_trace_radiance) on the MI355X: the render kernel shading caller-supplied
rays.  fp64 colours are within TOL64 = 1e-12 of the CPU oracle with equal ray counts, and equal
the render kernel's own frames bit for bit (the same operations)."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
import rtamd
from rtamd import abi

import query_cases as qc
import radiance_cases as rc

pytestmark = pytest.mark.gpu

TOL64 = rc.TOL64
W, H = 64, 48

_dev = {}


def _device(name, tree=None, **opt):
    """One upload per (scene, tree, options), shared by the tests of this module."""
    key = (name, tree, tuple(sorted(opt.items())))
    if key not in _dev:
        _dev[key] = rtamd.DeviceScene(rc.scene(name)[0], 0, tree=tree, **opt)
    return _dev[key]


def _frame(name):
    """(params, camera rays, oracle image, oracle counts) of the W x H frame of a scene."""
    hs, orc = rc.scene(name)
    p = rc.params(hs, W, H)
    ref, cnt = rc.oracle_frame((name, W, H), orc, p)
    return p, rtamd.camera_rays(p), ref, cnt


_whole = {}


def _whole_frame(name):
    """radiance of the whole W x H frame's camera rays on the default device scene, computed once."""
    if name not in _whole:
        p, rays, _, _ = _frame(name)
        _whole[name] = _device(name).radiance(rays, p)
    return _whole[name]


# ---- 1. camera rays equal the render ----
# (random_tris on the reference tree: the scene of tests/test_query_gpu.py that spills the 8-entry ring)
@pytest.mark.parametrize("name,tree,opt", [("cornell", None, {}), ("office", None, {}),
                                           ("random_tris", "reference", {}),
                                           ("office", None, {"stack_ring": 16}),
                                           ("random_tris", "reference", {"stack_ring": 16})])
def test_camera_rays_equal_the_render_and_the_oracle(gpu_available, name, tree, opt):
    p, rays, ref, cnt = _frame(name)
    dev = _device(name, tree, **opt)
    img, rst = dev.render(p)
    rgb, st = dev.radiance(rays, p, stats=True)
    assert rgb.shape == (W * H, 3) and rgb.dtype == np.float64
    assert np.array_equal(rgb.reshape(H, W, 3), img)
    assert np.abs(rgb.reshape(H, W, 3) - ref).max() <= TOL64
    assert rc.counts(st) == cnt == rc.counts(rst)
    assert st.pixels == W * H and st.node_visits == 0 and st.tri_tests == 0 and st.closest_hits == 0
    assert dev.status() == abi.RT_OK


# ---- 2. order independence ----
@pytest.mark.parametrize("name", ["office", "cornell"])
def test_ray_order_changes_no_colour_and_no_count(gpu_available, name):
    p, rays, ref, cnt = _frame(name)
    dev = _device(name)
    base, st0 = dev.radiance(rays, p, stats=True)
    for perm in (np.random.default_rng(3).permutation(W * H), rtamd.tile_major(W, H)):
        got, st = dev.radiance(rays[perm], p, stats=True)
        assert np.array_equal(got[np.argsort(perm)], base)
        assert rc.counts(st) == rc.counts(st0) == cnt


# ---- 3. partial waves and grid edges ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 3071])
def test_partial_waves_leave_the_rows_behind_untouched(gpu_available, n):
    import torch

    p, rays, ref, cnt = _frame("cornell")
    dev = _device("cornell")
    lib = rtamd.hip_lib()
    d_rays = torch.from_numpy(rays).cuda()
    out = torch.full((W * H, 3), -7.0, dtype=torch.float64, device="cuda")
    st = abi.Stats()
    assert lib.rt_trace_radiance(dev._h, C.byref(p), d_rays.data_ptr(), n, out.data_ptr(), C.byref(st), None) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], _whole_frame("cornell")[:n])   # the same rays in a full launch
    assert np.abs(got[:n] - ref.reshape(-1, 3)[:n]).max() <= TOL64
    assert np.all(got[n:] == -7.0)
    assert st.pixels == n and st.primary_rays == n
    # through the method, on a tensor of n rays
    rgb = dev.radiance(d_rays[:n].contiguous(), p)
    assert rgb.shape == (n, 3) and rgb.is_cuda and np.array_equal(rgb.cpu().numpy(), got[:n])


def test_zero_rays_launch_nothing_and_touch_nothing(gpu_available):
    import torch

    p, rays, _, _ = _frame("cornell")
    dev = _device("cornell")
    lib = rtamd.hip_lib()
    dev.render(p)
    grid = dev.last_grid()
    d_rays = torch.from_numpy(rays[:4]).cuda()
    out = torch.full((4, 3), -7.0, dtype=torch.float64, device="cuda")
    st = abi.Stats(primary_rays=-1, pixels=-1)
    assert lib.rt_trace_radiance(dev._h, C.byref(p), d_rays.data_ptr(), 0, out.data_ptr(), C.byref(st), None) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert (st.primary_rays, st.pixels) == (0, 0)
    assert dev.last_grid() == grid   # no launch was recorded
    got = dev.radiance(np.zeros((0, 8)), p)
    assert got.shape == (0, 3) and got.dtype == np.float64


# ---- 4. several origins in one call ----
def test_several_origins_in_one_call(gpu_available):
    hs, orc = rc.scene("office")
    base = rc.params(hs, 16, 16)
    lo, hi = qc.root_box(hs)
    eye0 = np.array(base.camera.eye[:])
    rng = np.random.default_rng(21)
    parts, refs, total = [], [], [0, 0, 0]
    for k in range(6):   # eyes inside the office: the camera's own eye pulled towards points of the box
        eye = eye0 + 0.3 * rng.random(3) * (lo + rng.random(3) * (hi - lo) - eye0)
        q = rc.with_eye(base, eye)
        ref, cnt = rc.oracle_frame(("office", "eye", k), orc, q)
        parts.append(rtamd.camera_rays(q))
        refs.append(ref.reshape(-1, 3))
        total = [a + b for a, b in zip(total, cnt)]
    rays, want = np.concatenate(parts), np.concatenate(refs)
    perm = np.random.default_rng(22).permutation(len(rays))
    got, st = _device("office").radiance(rays[perm], base, stats=True)
    assert np.abs(got - want[perm]).max() <= TOL64
    assert rc.counts(st) == total and st.pixels == 6 * 256


# ---- 5. arbitrary rays ----
def _arbitrary(name="office"):
    hs, orc = rc.scene(name)
    p = rc.params(hs, 8, 8)
    o, target, rays = rc.arbitrary_rays(hs)
    want, cnt = rc.oracle_single_rays((name, "arbitrary"), orc, p, o, target)
    hit, t = rc.hit_distances((name, "arbitrary", "t"), orc, rays)
    return p, rays, want, cnt, hit, t


def test_arbitrary_rays_match_single_pixel_oracle_renders(gpu_available):
    p, rays, want, cnt, hit, t = _arbitrary()
    assert hit.sum() >= 16 and (~hit).sum() >= 16   # hits and misses are both in the set
    got, st = _device("office").radiance(rays, p, stats=True)
    assert np.abs(got - want).max() <= TOL64
    assert rc.counts(st) == cnt and cnt[0] == 256
    assert np.all(got[~hit] == rc.background(p))


# ---- 6. tmax ----
def test_tmax_bounds_the_primary_segment_only(gpu_available):
    p, rays, want, cnt, hit, t = _arbitrary()
    dev = _device("office")
    free = dev.radiance(rays, p)
    r = rays[hit].copy()
    r[:, 6] = np.nextafter(t[hit], np.inf)
    assert np.array_equal(dev.radiance(r, p), free[hit])
    for tmax in (t[hit], 0.5 * t[hit]):
        r[:, 6] = tmax
        got, st = dev.radiance(r, p, stats=True)
        assert np.all(got == rc.background(p))
        assert rc.counts(st) == [int(hit.sum()), 0, 0]
    big = rays.copy()
    big[:, 6] = np.finfo(np.float64).max
    assert np.array_equal(dev.radiance(big, p), free)


# ---- 7. degenerate rays ----
def test_degenerate_rays_get_the_background_and_are_not_counted(gpu_available):
    p, rays, want, cnt, hit, t = _arbitrary()
    dev = _device("office")
    good = rays[hit][:48]
    alone, st0 = dev.radiance(good, p, stats=True)
    bad = rc.degenerate_rows(good[:16])
    mixed = np.concatenate([bad, good])
    perm = np.random.default_rng(9).permutation(len(mixed))   # degenerate rays among the valid ones
    got, st = dev.radiance(mixed[perm], p, stats=True)
    got = got[np.argsort(perm)]
    assert np.all(got[:len(bad)] == rc.background(p))
    assert np.array_equal(got[len(bad):], alone)
    assert rc.counts(st) == rc.counts(st0) and st.primary_rays == len(good)
    assert st.pixels == len(mixed)
    only_bad, sb = dev.radiance(bad, p, stats=True)   # a launch that never traverses
    assert np.all(only_bad == rc.background(p)) and rc.counts(sb) == [0, 0, 0]
    assert dev.status() == abi.RT_OK


# ---- 8. analytic primitives ----
def test_analytic_primitives(gpu_available):
    hs = rtamd.HostScene.generate("spheres")
    hs.prepare()
    orc = pyoracle.Oracle(hs.raw, hs)
    dev = rtamd.DeviceScene(hs, 0, analytic=True)
    p = rc.params(hs, 32, 24)
    ref, cnt = orc.render(p, rc.REF)
    img, rst = dev.render(p)
    rgb, st = dev.radiance(rtamd.camera_rays(p), p, stats=True)
    assert np.array_equal(rgb.reshape(24, 32, 3), img)
    assert np.abs(rgb.reshape(24, 32, 3) - ref).max() <= TOL64
    assert rc.counts(st) == [cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays]
    assert st.shadow_rays > 0 and st.reflection_rays > 0
    dev.close()


# ---- 9. lights ----
def test_seventeen_lights_then_two(gpu_available):
    hs, orc = rc.scene("cornell")
    dev = _device("cornell")
    p2 = rc.params(hs, 32, 24)
    assert p2.n_lights >= 2
    p2.n_lights = 2
    base = [(tuple(p2.lights[i].position), tuple(p2.lights[i].color)) for i in range(2)]
    p17 = rc.params(hs, 32, 24)
    lights = []
    for i in range(17):
        a = 2.0 * np.pi * i / 17
        pos, _ = base[i % 2]
        lights.append(((pos[0] + 0.3 * np.cos(a), pos[1], pos[2] + 0.3 * np.sin(a)), (0.1 + 0.02 * (i % 5),) * 3))
    p17.set_lights(lights)
    assert p17.n_lights == 17 and bool(p17.lights_ext)
    rays = rtamd.camera_rays(p2)
    for p in (p17, p2):   # the light table is copied with every launch: 2 lights after 17
        ref, cnt = orc.render(p, rc.REF)
        rgb, st = dev.radiance(rays, p, stats=True)
        assert np.abs(rgb.reshape(24, 32, 3) - ref).max() <= TOL64
        assert rc.counts(st) == [cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays]


# ---- 10. f32 output ----
def test_f32_output_is_the_rounded_f64_result(gpu_available):
    p, rays, _, _ = _frame("office")
    dev = _device("office")
    rgb64 = dev.radiance(rays, p)
    rgb32 = dev.radiance(rays, rc.copy_params(p, out_format=rtamd.RT_OUT_RGB_F32))
    assert rgb32.dtype == np.float32 and np.array_equal(rgb32, rgb64.astype(np.float32))


# ---- 11. beside a render ----
def test_radiance_beside_a_render_on_another_stream(gpu_available):
    import torch

    hs, _ = rc.scene("office")
    dev = _device("office")
    p, rays, _, _ = _frame("office")
    d_rays = torch.from_numpy(rays).cuda()
    pf = rc.params(hs, 96, 54)
    serial_rgb = dev.radiance(d_rays, p).clone()
    serial = torch.zeros((20, 54, 96, 3), dtype=torch.float64, device="cuda")
    dev.launch_frames(pf, [serial[f].data_ptr() for f in range(20)])
    torch.cuda.synchronize()
    frames = torch.zeros_like(serial)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dev.launch_frames(pf, [frames[f].data_ptr() for f in range(20)], stream=s1.cuda_stream)
    got = dev.radiance(d_rays, p, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert bool((got == serial_rgb).all())
    assert bool((frames == serial).all())
    assert dev.status() == abi.RT_OK


# ---- 12. renders undisturbed ----
def test_frame_launches_behave_as_if_the_radiance_call_had_not_happened(gpu_available):
    """Two one-frame launches of one camera on the null stream (cost-ordered by default: costs are
    recorded), a radiance call, a third launch: three bit-identical images, and the third launch
    continues the cost-order sequence.  The first launch a sequence orders is its third, so the
    length rt_debug_last_tile_order reports after the second launch (0 on a fresh scene) cannot equal
    the one after the third; the sequence is compared with a control scene that gets no radiance call
    instead: the same lengths after the second and the third launch, the third a permutation."""
    hs, _ = rc.scene("cornell")
    lib = rtamd.hip_lib()
    p, rays, ref, _ = _frame("cornell")
    tw, th = rtamd.tile_shape()
    n_tiles = -(-W // tw) * -(-H // th)

    def order_len(dev):
        return int(lib.rt_debug_last_tile_order(dev._h, None, 0))

    seen = {}
    for with_radiance in (False, True):
        dev = rtamd.DeviceScene(hs, 0)
        a, _ = dev.render(p)
        b, _ = dev.render(p)
        m2 = order_len(dev)
        if with_radiance:
            rgb = dev.radiance(rays, p)
            assert np.array_equal(rgb.reshape(H, W, 3), a)
            assert order_len(dev) == m2
        c, _ = dev.render(p)
        m3 = order_len(dev)
        assert np.array_equal(a, b) and np.array_equal(a, c)
        got = np.zeros(max(1, m3), dtype=np.uint32)
        lib.rt_debug_last_tile_order(dev._h, got.ctypes.data_as(C.POINTER(C.c_uint)), m3)
        assert m3 == n_tiles and np.array_equal(np.sort(got[:m3]), np.arange(n_tiles))
        seen[with_radiance] = (m2, m3)
        dev.close()
    assert seen[True] == seen[False]


# ---- 13. panorama ----
def test_panorama_rays_end_to_end(gpu_available):
    hs, orc = rc.scene("office")
    p = rc.params(hs, 96, 54)
    rays = rtamd.panorama_rays(p, 32, 16)
    o = rays[:, 0:3]
    want, cnt = rc.oracle_single_rays(("office", "panorama"), orc, p, o, o + rays[:, 3:6])
    # the oracle's direction is (o + d) - o: the rays under test are the same subtraction
    rays[:, 3:6] = (o + rays[:, 3:6]) - o
    got, st = _device("office").radiance(rays, p, stats=True)
    assert np.abs(got - want).max() <= TOL64
    assert rc.counts(st) == cnt and st.pixels == 512
