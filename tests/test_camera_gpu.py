"""A camera's hits and surface points made on the device (DeviceScene.camera: rt_trace_camera,
DESIGN.md §22).  The reference of every case is the written-out chain: rt_trace_closest of
camera_rays_host(params, order) -- the entry point test_query_gpu.py pins to the oracle -- and
surface_points_host of its rows.  Every comparison is exact: raw 64-B rows, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
import rtamd
from rtamd import abi

import ao_cases
import camera_cases as cc
import fuzz_scenes
import query_cases as qc

pytestmark = pytest.mark.gpu

SPILL_SCENE = ("random_tris", 20000, "reference")   # test_query_gpu.py's
SCENES = [("cornell", None), ("office", None), ("random_tris", "reference")]
GUARD = 0x5a5a5a5a
# (hits, misses, flipped normals) of the reference, measured with the CPU oracle
COUNTS = {("cornell", 32, 24): (484, 284, 41), ("cornell", 13, 11): (100, 43, 9),
          ("random_tris", 32, 24): (367, 401, 187), ("random_tris", 13, 11): (73, 70, 33),
          ("office", 32, 24): (768, 0, 11)}

_dev, _ref = {}, {}


def _scene(name):
    return qc.scene(name, qc.SCENES[name].get("n_triangles", 0))


def _device(name, tree):
    """One upload per (scene, tree), shared by the tests of this module."""
    if (name, tree) not in _dev:
        _dev[(name, tree)] = rtamd.DeviceScene(_scene(name)[0], 0, tree=tree)
    return _dev[(name, tree)]


def _closest_rows(dev, rays):
    """rt_trace_closest of host rays: the raw [n, 8] float64 rt_hit rows, and its hit counter."""
    import torch

    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    out = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    st = abi.QueryStats()
    rc = rtamd.hip_lib().rt_trace_closest(dev._h, d_rays.data_ptr(), n, out.data_ptr(), C.byref(st), None)
    assert rc == abi.RT_OK, rtamd.hip_lib().rt_last_error()
    return out.cpu().numpy(), int(st.hits)


def _reference(dev, p, order, point_tmax=np.inf):
    """(rays, rt_hit rows, point records) of the written-out chain."""
    rays = rtamd.camera_rays_host(p, order)
    rows, nhit = _closest_rows(dev, rays)
    assert nhit == int((rows[:, 0] < np.inf).sum())
    return rays, rows, rtamd.surface_points_host(rays, rows, point_tmax)


def _shared_reference(name, tree, W, H, order):
    """The reference of a full frame, computed once and shared; callers must not modify it."""
    key = (name, tree, W, H, order)
    if key not in _ref:
        _ref[key] = _reference(_device(name, tree), cc.params(_scene(name)[0], W, H), order)
    return _ref[key]


def _rows(views):
    """The [n, 8] float64 tensor behind the views DeviceScene.camera / trace return, as numpy."""
    base = views["t"]._base
    assert base is not None and base.dim() == 2 and base.shape[1] == 8
    for k in ("alpha", "beta", "normal", "slot", "mesh", "prim"):
        assert views[k].data_ptr() - base.data_ptr() in (8, 16, 24, 48, 52, 56)
    return base.cpu().numpy()


def _same_rows(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check(dev, p, order, want, point_tmax=np.inf):
    """camera() with hits and points against the reference, raw rows; returns the stats."""
    _, rows, pts = want
    got, st = dev.camera(p, hits=True, points=True, order=order, point_tmax=point_tmax, stats=True)
    g_rows, g_pts = _rows(got["hits"]), got["points"].cpu().numpy()
    n = len(rows)
    nhit = int((rows[:, 0] < np.inf).sum())
    print(f"{p.camera.width} x {p.camera.height} {order}: n {n} hits {nhit}, differing hit rows "
          f"{int((g_rows.view(np.uint64) != rows.view(np.uint64)).any(1).sum()) if g_rows.shape == rows.shape else -1}, "
          f"spills {st.stack_spills}")
    assert _same_rows(g_rows, rows)
    assert _same_rows(g_pts, pts)
    assert (st.rays, st.hits, st.watchdog) == (n, nhit, 0)
    assert dev.status() == abi.RT_OK
    return st


@pytest.mark.parametrize("order", cc.ORDERS)
@pytest.mark.parametrize("W,H", [(32, 24), (13, 11)])
@pytest.mark.parametrize("name,tree", SCENES)
def test_hits_and_points_equal_the_written_out_chain(gpu_available, name, tree, W, H, order):
    dev = _device(name, tree)
    want = _shared_reference(name, tree, W, H, order)
    rays, rows, pts = want
    # the reference itself shows the ground this claims to cover
    hit = rows[:, 0] < np.inf
    flip = cc.flipped(rays, rows)
    counts = (int(hit.sum()), int((~hit).sum()), int(flip.sum()))
    print(f"{name} {W} x {H}: hits, misses, flipped = {counts}")
    if (name, W, H) in COUNTS:
        assert counts == COUNTS[(name, W, H)]
    if name != "office":
        assert hit.any() and (~hit).any()
    assert flip.any()
    assert cc.same_bits(pts, cc.numpy_points(rays, rows))
    _check(dev, cc.params(_scene(name)[0], W, H), order, want)


@pytest.mark.parametrize("order", cc.ORDERS)
@pytest.mark.parametrize("W,H", [(9, 1), (1, 9), (1, 1), (8, 8), (64, 1)])
def test_small_cameras(gpu_available, W, H, order):
    dev = _device("cornell", None)
    p = cc.params(_scene("cornell")[0], W, H)
    _check(dev, p, order, _reference(dev, p, order))


@pytest.mark.parametrize("name,tree,W,H", [("cornell", None, 32, 24), ("random_tris", "reference", 13, 11)])
def test_hits_equal_the_cpu_oracle(gpu_available, name, tree, W, H):
    hs, orc, P, vidx, perm = _scene(name)
    dev = _device(name, tree)
    p = cc.params(hs, W, H)
    rays = rtamd.camera_rays_host(p, "row")
    want = qc.expected(("camera", name, W, H), orc, rays, pyoracle.MODE_REFERENCE)
    got = {k: v.cpu().numpy() for k, v in dev.camera(p)["hits"].items()}
    assert int(want["hit"].sum()) == COUNTS[(name, W, H)][0]
    qc.check_hits(got, want, rays, P, vidx, perm)
    # ... and the points carry the oracle's normals, some of them turned round
    pts = dev.camera(p, hits=False, points=True)["points"].cpu().numpy()
    h = want["hit"]
    assert np.array_equal(np.abs(pts[h, 3:6]), np.abs(want["normal"][h]))
    assert int((pts[h, 3:6] != want["normal"][h]).any(1).sum()) == COUNTS[(name, W, H)][2]


@pytest.mark.parametrize("order", cc.ORDERS)
@pytest.mark.parametrize("shard", sorted(cc.SHARDS))
def test_shards(gpu_available, shard, order):
    hs = _scene("cornell")[0]
    dev = _device("cornell", None)
    p = cc.params(hs, 32, 24, **cc.SHARDS[shard])
    want = _reference(dev, p, order)
    assert len(want[0]) == 32 * len(cc.shard_rows(p))
    _check(dev, p, order, want)
    if order == "row":   # the shard's records are the full frame's records of its rows
        full = _shared_reference("cornell", None, 32, 24, "row")[1].reshape(24, 32, 8)
        assert _same_rows(want[1], full[cc.shard_rows(p)].reshape(-1, 8))


def test_a_row_range_with_stripes_is_refused_as_by_the_render_launch(gpu_available):
    import torch

    hs = _scene("cornell")[0]
    dev = _device("cornell", None)
    p = cc.params(hs, 32, 24, **cc.SHARD_REFUSED)
    with pytest.raises(rtamd.RtError) as e:
        dev.camera(p)
    assert "row ranges cannot be combined" in str(e.value)
    out = torch.zeros((32 * 24, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(rtamd.RtError) as e:
        dev.launch(p, out.data_ptr())
    assert "row ranges cannot be combined" in str(e.value)


@pytest.mark.parametrize("order", cc.ORDERS)
@pytest.mark.parametrize("hits,points", [(True, False), (False, True), (True, True)])
def test_output_selection_and_guards(gpu_available, hits, points, order):
    import torch

    dev = _device("cornell", None)
    p = cc.params(_scene("cornell")[0], 13, 11)
    n = 13 * 11
    _, rows, pts = _shared_reference("cornell", None, 13, 11, order)
    bufs = [torch.full(((n + 64) * 16,), GUARD, dtype=torch.int32, device="cuda") for _ in range(2)]
    out = abi.CameraOut(d_hits=bufs[0].data_ptr() if hits else None, d_points=bufs[1].data_ptr() if points else None,
                        order=abi.RT_CAMERA_TILE_MAJOR if order == "tile" else abi.RT_CAMERA_ROW_MAJOR,
                        point_tmax=float("inf"))
    st = abi.QueryStats()
    rc = rtamd.hip_lib().rt_trace_camera(dev._h, C.byref(p), C.byref(out), C.byref(st), None)
    assert rc == abi.RT_OK, rtamd.hip_lib().rt_last_error()
    for buf, asked, want in ((bufs[0], hits, rows), (bufs[1], points, pts)):
        got = buf.cpu().numpy()
        if asked:
            assert _same_rows(got[:n * 16].view(np.float64).reshape(n, 8), want)
            assert np.all(got[n * 16:] == GUARD)
        else:
            assert np.all(got == GUARD)
    assert (st.rays, st.hits) == (n, COUNTS[("cornell", 13, 11)][0])
    # the Python layer returns what was asked for
    res = dev.camera(p, hits=hits, points=points, order=order)
    assert set(res) == ({"hits"} if hits else set()) | ({"points"} if points else set())
    if hits:
        assert _same_rows(_rows(res["hits"]), rows) and res["hits"]["slot"].dtype == torch.int32
    if points:
        assert res["points"].is_cuda and _same_rows(res["points"].cpu().numpy(), pts)


def test_stats_and_the_stack_spill_path(gpu_available):
    name, n_tri, tree = SPILL_SCENE
    assert qc.SCENES[name]["n_triangles"] == n_tri
    dev = _device(name, tree)
    for order in cc.ORDERS:
        st = _check(dev, cc.params(_scene(name)[0], 32, 24), order, _shared_reference(name, tree, 32, 24, order))
        print(f"spill scene {order}: stack_spills {st.stack_spills}")
        assert st.stack_spills > 0   # without it this test proves nothing about the spill path
        assert (st.rays, st.hits) == (768, COUNTS[(name, 32, 24)][0])
    # without stats the call returns at once and the counters stay the caller's
    got = dev.camera(cc.params(_scene(name)[0], 32, 24))
    assert _same_rows(_rows(got["hits"]), _shared_reference(name, tree, 32, 24, "row")[1])
    assert dev.status() == abi.RT_OK


@pytest.mark.parametrize("order", cc.ORDERS)
def test_point_tmax_lands_in_every_record(gpu_available, order):
    dev = _device("cornell", None)
    p = cc.params(_scene("cornell")[0], 32, 24)
    rays, rows, _ = _shared_reference("cornell", None, 32, 24, order)
    want = rtamd.surface_points_host(rays, rows, 2.5)
    got = dev.camera(p, hits=False, points=True, order=order, point_tmax=2.5)["points"].cpu().numpy()
    assert _same_rows(got, want)
    miss = ~(rows[:, 0] < np.inf)
    assert miss.any() and np.all(got[:, 6] == 2.5) and np.all(got[:, 7] == 0.0)
    assert np.all(got[miss, 3:6] == 0.0) and cc.same_bits(got[miss, 0:3], rays[miss, 0:3])
    with pytest.raises(rtamd.RtError):
        dev.camera(p, points=True, point_tmax=1e-5)
    with pytest.raises(rtamd.RtError):
        dev.camera(p, points=True, point_tmax=float("nan"))
    assert "hits" in dev.camera(p, point_tmax=float("nan"))   # not read without points


def test_analytic_primitives(gpu_available, tmp_path):
    hs = rtamd.HostScene.load(fuzz_scenes.write_analytic(tmp_path, 3, 64, 48))
    hs.prepare()
    assert hs.raw.contents.n_spheres >= 1
    dev = rtamd.DeviceScene(hs, 0, analytic=True)
    plain = rtamd.DeviceScene(hs, 0)
    p = cc.params(hs, 32, 24)
    for order in cc.ORDERS:
        want = _reference(dev, p, order)
        _check(dev, p, order, want)
        prim = want[1].view(np.int32).reshape(-1, 16)[:, 14]
        assert (prim >= 0).sum() > 0 and (prim < 0).sum() > 0
        got = dev.camera(p, order=order)["hits"]
        assert np.array_equal(got["prim"].cpu().numpy(), prim)
    # the primitives take part: without them the frame differs
    assert not _same_rows(_rows(plain.camera(p)["hits"]), _reference(dev, p, "row")[1])
    dev.close()
    plain.close()


def test_camera_beside_a_render_on_another_stream(gpu_available):
    import torch

    hs = _scene("office")[0]
    dev = _device("office", None)
    q = cc.params(hs, 32, 24)
    _, rows, pts = _shared_reference("office", None, 32, 24, "tile")
    p = hs.render_params(96, 54, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    serial = torch.zeros((20, 54, 96, 3), dtype=torch.float64, device="cuda")
    dev.launch_frames(p, [serial[f].data_ptr() for f in range(20)])
    torch.cuda.synchronize()
    frames = torch.zeros_like(serial)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dev.launch_frames(p, [frames[f].data_ptr() for f in range(20)], stream=s1.cuda_stream)
    got = dev.camera(q, hits=True, points=True, order="tile", stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert _same_rows(_rows(got["hits"]), rows) and _same_rows(got["points"].cpu().numpy(), pts)
    assert bool((frames == serial).all())
    assert dev.status() == abi.RT_OK


def test_repeatable(gpu_available):
    dev = _device("office", None)
    q = cc.params(_scene("office")[0], 32, 24)
    a = dev.camera(q, hits=True, points=True, order="tile")
    b = dev.camera(q, hits=True, points=True, order="tile")
    assert _same_rows(_rows(a["hits"]), _rows(b["hits"]))
    assert _same_rows(a["points"].cpu().numpy(), b["points"].cpu().numpy())


def _half_diagonal(dev):
    lo, hi = dev.bounds()
    e = hi - lo
    return 0.5 * np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])


def _ao_reference(dev, name, tree, dirs, seed, bias, radius):
    """The composition on the written-out chain's points: tile-major records -> ao -> image order."""
    rays, rows, _ = _shared_reference(name, tree, 32, 24, "tile")
    pts = rtamd.surface_points_host(rays, rows, radius)
    counts = dev.ao(pts, dirs, seed=seed, bias=bias)
    img = np.zeros(32 * 24, dtype=np.int64)
    img[rtamd.tile_major(32, 24)] = counts
    return img


def test_ao_image(gpu_available):
    """ao_image against ao() on the reference's points, exactly.  A point's direction set is
    hash(record index ^ seed) % n_sets (rt_trace_ao), and ao_image's records are in tile order: with
    4 sets it equals ao() of the row-order points at every pixel whose set is the same under both
    indices, and at every pixel with one set."""
    import torch

    dev = _device("cornell", None)
    p = cc.params(_scene("cornell")[0], 32, 24)
    k, n_sets, seed, bias = 16, 4, 3, 1e-6
    dirs = rtamd.ao_directions(k, n_sets, seed=1)
    got = dev.ao_image(p, dirs, seed=seed, bias=bias)
    assert got.shape == (24, 32) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    want = _ao_reference(dev, "cornell", None, dirs, seed, bias, np.inf)
    assert np.array_equal(got, (want / float(k)).reshape(24, 32))
    assert np.any(want == 0) and np.any(want == k) and np.any((want > 0) & (want < k))
    # the surface points in row order, literally
    rays, rows, pts = _shared_reference("cornell", None, 32, 24, "row")
    row_counts = dev.ao(pts, dirs, seed=seed, bias=bias)
    perm = rtamd.tile_major(32, 24)
    set_row = ao_cases.numpy_sets(768, seed, n_sets)
    set_tile = np.zeros(768, dtype=set_row.dtype)
    set_tile[perm] = ao_cases.numpy_sets(768, seed, n_sets)   # the set of the pixel's tile-order record
    same = set_row == set_tile
    print(f"ao_image: {int(same.sum())} of 768 pixels keep their set, "
          f"{int((got.ravel() * k != row_counts).sum())} pixels differ from the row-order call")
    assert 100 < same.sum() < 668
    assert np.array_equal(got.ravel()[same], row_counts[same] / float(k))
    one = dev.ao_image(p, dirs[:1], seed=seed, bias=bias).cpu().numpy()
    assert np.array_equal(one, (dev.ao(pts, dirs[:1], seed=seed, bias=bias) / float(k)).reshape(24, 32))


def test_ao_image_with_a_radius(gpu_available):
    dev = _device("office", None)
    p = cc.params(_scene("office")[0], 32, 24)
    k = 16
    dirs = rtamd.ao_directions(k, 4, seed=2)
    r = _half_diagonal(dev)
    want = _ao_reference(dev, "office", None, dirs, 5, 1e-6, r)
    assert np.any((want > 0) & (want < k))   # partly open: the closed room with a bounded fan
    got = dev.ao_image(p, dirs, seed=5, bias=1e-6, radius=r).cpu().numpy()
    assert np.array_equal(got, (want / float(k)).reshape(24, 32))
    # the unbounded fan sees nothing but walls there
    assert np.all(dev.ao_image(p, dirs, seed=5, bias=1e-6).cpu().numpy() == 0.0)


@pytest.mark.parametrize("fmt", ["f64", "f32"])
def test_gather_image(gpu_available, fmt):
    import torch

    dev = _device("cornell", None)
    p = cc.params(_scene("cornell")[0], 32, 24)
    p.out_format = rtamd.RT_OUT_RGB_F64 if fmt == "f64" else rtamd.RT_OUT_RGB_F32
    dirs = rtamd.ao_directions(16, 4, seed=1)
    got = dev.gather_image(p, dirs, seed=3, bias=1e-6)
    assert got.shape == (24, 32, 3) and got.dtype == (torch.float64 if fmt == "f64" else torch.float32)
    rays, rows, pts = _shared_reference("cornell", None, 32, 24, "tile")
    rgb = dev.gather(pts, dirs, p, seed=3, bias=1e-6)
    want = np.zeros_like(rgb)
    want[rtamd.tile_major(32, 24)] = rgb
    got = got.cpu().numpy().reshape(-1, 3)
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert len(np.unique(want, axis=0)) > 100
    # the pixels that see the background all report one colour
    miss = np.zeros(768, bool)
    miss[rtamd.tile_major(32, 24)] = ~(rows[:, 0] < np.inf)
    assert miss.sum() == COUNTS[("cornell", 32, 24)][1] and len(np.unique(got[miss], axis=0)) == 1


def test_python_layer_checks_its_inputs(gpu_available):
    dev = _device("cornell", None)
    p = cc.params(_scene("cornell")[0], 13, 11)
    with pytest.raises(ValueError):
        dev.camera(p, order="morton")
    with pytest.raises(ValueError):
        dev.camera(p, hits=False, points=False)
    p.spp_n = 2
    with pytest.raises(rtamd.RtError):
        dev.camera(p)
    empty = cc.params(_scene("cornell")[0], 13, 11, row_begin=4, row_end=4)
    res = dev.camera(empty, hits=True, points=True)
    assert res["points"].shape == (0, 8) and res["hits"]["t"].shape == (0,)
