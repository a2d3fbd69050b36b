"""rt_scene_update_positions on the device (include/rt_hip.h): a scene moved by
positions alone, from a numpy array (host path) and from a device tensor (device path).  The face
and vertex normals, max|vertex| and the root box are made by kernels.

The definition is compositional, and so is every check: a twin scene, uploaded from the same host
scene with the same options, is moved through the host path (HostScene.update_vertices +
DeviceScene.update), and the device's 4-wide nodes, triangle records and normal records
(rt_debug_scene_image), rt_scene_bounds, fp64 frames and ray counts are compared with ==, byte for
byte.  Scenes: update_cases' fuzz seeds (under 256 vertices: one partial block), cornell and office
(several blocks, a ragged last one), positions_cases' `fan` (the long CSR walk, an unreferenced
vertex that decides delta) and `degenerate`."""
import ctypes as C

import numpy as np
import pytest

import positions_cases as pc
import query_cases as qc
import radiance_cases as rc
import rtamd
import update_cases as uc
from rtamd import abi

pytestmark = pytest.mark.gpu

IMAGES = ("nodes4", "tris", "tnorm")
MODES = (("sbvh", True), ("sbvh", False), ("sah", False))   # (tree, reclip)


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    return gpu_available


def _params(hs, key, flags=0):
    w, h = pc.frame_size(key)
    p = hs.render_params(w, h, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    p.flags = flags
    return p


def _images(dev):
    return {k: dev.debug_scene_image(k) for k in IMAGES}


def _same_images(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in IMAGES)


def _same_bounds(a, b):
    return all(np.array_equal(pc.bits(x), pc.bits(y)) for x, y in zip(a.bounds(), b.bounds()))


def _tensor(pos):
    import torch
    return torch.from_numpy(np.ascontiguousarray(pos)).to("cuda:0")


def _scene(hs, tree, **options):
    dev = rtamd.DeviceScene(hs, 0, tree=tree, **options)
    dev.set_triangle_order(hs.slot_triangles())
    return dev


def _same_hits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("t", "alpha", "beta", "normal", "slot", "mesh", "prim"))


# ---- images, bounds, frames ----
@pytest.mark.parametrize("tree,reclip", MODES)
@pytest.mark.parametrize("key", pc.KEYS, ids=lambda k: f"{k[0]}-{k[1]}")
def test_images_bounds_and_frames_equal_the_host_path(key, tree, reclip):
    hs, posB = pc.case(key)
    twin = rtamd.DeviceScene(hs, 0, tree=tree)
    from_host, from_dev = _scene(hs, tree), _scene(hs, tree)
    p = _params(hs, key)
    before = _images(twin)
    assert _same_images(before, _images(from_host))
    from_host.update_positions(posB, reclip=reclip)
    from_dev.update_positions(_tensor(posB), reclip=reclip)
    hs.update_vertices(posB)                     # the host path, afterwards: the calls above need no host scene
    twin.update(hs, reclip=reclip)
    want = _images(twin)
    assert not np.array_equal(want["tris"], before["tris"])
    frame, st = twin.render(p)
    for dev in (from_host, from_dev):
        assert _same_images(_images(dev), want)
        assert _same_bounds(dev, twin)
        img, got = dev.render(p)
        assert np.array_equal(pc.bits(img), pc.bits(frame))
        assert rc.counts(got) == rc.counts(st) and got.pixels == st.pixels
        dev.close()
    assert len(np.unique(frame.reshape(-1, 3), axis=0)) > 2
    twin.close()


def test_fresh_upload_and_closest_hits():
    key = ("fuzz", uc.KEPT[0])
    hs, posB = pc.case(key)
    dev = _scene(hs, None)
    dev.update_positions(_tensor(posB), reclip=True)
    hs.update_vertices(posB)
    fresh = rtamd.DeviceScene(hs, 0)
    p = _params(hs, key)
    img, st = dev.render(p)
    want, wst = fresh.render(p)
    assert np.array_equal(pc.bits(img), pc.bits(want)) and rc.counts(st) == rc.counts(wst)
    rays = np.concatenate([qc.random_rays(hs, 512), qc.vertex_rays(hs, posB, 512)])
    got, qs = dev.trace(rays, stats=True)
    ref, rs = fresh.trace(rays, stats=True)
    assert _same_hits(got, ref) and qs.hits == rs.hits >= 64 and qs.watchdog == 0
    assert np.array_equal(dev.trace(rays, occluded=True), fresh.trace(rays, occluded=True))
    assert _same_bounds(dev, fresh)
    dev.close()
    fresh.close()


# ---- alternation ----
def test_the_two_update_calls_alternate():
    key = ("gen", "cornell")
    hs, posB = pc.case(key)
    posA = hs.soa_arrays()["vertex_pos"].copy()
    dev, twin = _scene(hs, "sbvh"), rtamd.DeviceScene(hs, 0, tree="sbvh")
    hs.update_vertices(posB)
    dev.update(hs, reclip=True)                              # 1: host path to B
    first = _images(dev)
    dev.update_positions(_tensor(posA), reclip=True)         # 2: back to A from a device tensor
    hs.update_vertices(posA)
    twin.update(hs, reclip=True)
    assert _same_images(_images(dev), _images(twin)) and _same_bounds(dev, twin)
    hs.update_vertices(posB)
    dev.update(hs, reclip=True)                              # 3: host path to B again
    assert _same_images(_images(dev), first)
    assert not _same_images(first, _images(twin))
    dev.close()
    twin.close()


# ---- queued work ----
def test_host_pointer_updates_and_renders_queued_on_one_stream():
    import torch

    key = ("fuzz", uc.KEPT[1])
    hs, posB = pc.case(key)
    posA = hs.soa_arrays()["vertex_pos"].copy()
    posC = 0.5 * (posA + posB)
    dev = _scene(hs, None)
    p = _params(hs, key)
    outs = [torch.zeros((uc.H, uc.W, 3), dtype=torch.float64, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    scratch = posB.copy()
    dev.update_positions(scratch, stream=stream.cuda_stream, reclip=True)   # no host synchronisation in between
    scratch[:] = np.nan                                                     # the array may be reused at once
    dev.launch(p, outs[0].data_ptr(), stream=stream.cuda_stream)
    dev.update_positions(posC, stream=stream.cuda_stream, reclip=True)
    dev.launch(p, outs[1].data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    got = [o.cpu().numpy() for o in outs]
    twin = rtamd.DeviceScene(hs, 0)
    for pos, img in zip((posB, posC), got):
        hs.update_vertices(pos)
        twin.update(hs, reclip=True)
        assert np.array_equal(pc.bits(img), pc.bits(twin.render(p)[0]))
    assert not np.array_equal(got[0], got[1])
    dev.close()
    twin.close()


# ---- refusal ----
def test_device_tensor_beyond_the_range_is_refused_and_changes_nothing():
    key = ("gen", "cornell")
    hs, posB = pc.case(key)
    dev = _scene(hs, "sbvh")
    dev.update_positions(_tensor(posB), reclip=True)     # (first use: the allocations are behind us)
    p = _params(hs, key)
    img, st = dev.render(p)
    images, bounds, b0 = _images(dev), dev.bounds(), dev.device_bytes
    bad = hs.soa_arrays()["vertex_pos"].copy()
    bad[len(bad) // 2, 1] = -2.0 * abi.RT_MAX_COORDINATE
    t = _tensor(bad)
    with pytest.raises(rtamd.RtError, match="coordinate"):
        dev.update_positions(t, reclip=True)
    pos = abi.ScenePositions(n_vertices=len(bad), vertex_pos=t.data_ptr(), on_device=1)
    assert rtamd.hip_lib().rt_scene_update_positions(dev._h, C.byref(pos), 0, None) == abi.RT_ERR_UNSUPPORTED
    with pytest.raises(rtamd.RtError, match="coordinate"):
        dev.update_positions(bad)                        # the host path refuses it too
    assert _same_images(_images(dev), images)
    assert all(np.array_equal(pc.bits(a), pc.bits(b)) for a, b in zip(dev.bounds(), bounds))
    img2, st2 = dev.render(p)
    assert np.array_equal(pc.bits(img2), pc.bits(img)) and rc.counts(st2) == rc.counts(st)
    assert dev.device_bytes == b0
    bad[len(bad) // 2, 1] = -abi.RT_MAX_COORDINATE       # the limit itself is taken
    dev.update_positions(_tensor(bad))
    dev.close()


def test_argument_checks_on_a_real_scene():
    import torch

    hs, posB = pc.case(("made", "degenerate"))
    dev = rtamd.DeviceScene(hs, 0)
    with pytest.raises(rtamd.RtError, match="rt_scene_set_triangle_order"):
        dev.update_positions(posB)
    order = hs.slot_triangles()
    with pytest.raises(rtamd.RtError, match="n_triangles"):
        dev.set_triangle_order(order[:-1].argsort().argsort().astype(np.int32))
    twice = order.copy()
    twice[0] = twice[1]
    with pytest.raises(rtamd.RtError, match="permutation"):
        dev.set_triangle_order(twice)
    dev.set_triangle_order(order)
    with pytest.raises(rtamd.RtError, match="n_vertices"):
        dev.update_positions(posB[:-1])
    with pytest.raises(rtamd.RtError, match="n_vertices"):
        dev.update_positions(_tensor(posB[:-1]))
    for bad in (_tensor(posB).to(torch.float32), _tensor(posB).t(), _tensor(posB).reshape(-1), torch.from_numpy(posB)):
        with pytest.raises(ValueError):
            dev.update_positions(bad)
    dev.update_positions(posB)
    dev.close()


# ---- device bytes ----
def test_device_bytes_grow_by_the_documented_amounts():
    hs, posB = pc.case(("gen", "cornell"))
    soa = hs.soa_arrays()
    nv, nt = len(soa["vertex_pos"]), len(soa["vertex_idx"])
    n_used = len(np.unique(soa["vertex_idx"]))
    dev, twin = rtamd.DeviceScene(hs, 0), rtamd.DeviceScene(hs, 0)
    b0 = dev.device_bytes
    assert twin.device_bytes == b0
    dev.set_triangle_order(hs.slot_triangles())
    b1 = dev.device_bytes
    assert b1 - b0 == 60 * nt + 4 * (nv + 1)
    dev.set_triangle_order(hs.slot_triangles())          # again: the tables are replaced
    assert dev.device_bytes == b1
    hs.update_vertices(posB)
    twin.update(hs, reclip=True)
    first_update = twin.device_bytes - b0                # what rt_scene_update_vertices allocates
    assert first_update > 0
    dev.update_positions(posB, reclip=True)              # the host path adds nothing of its own
    assert dev.device_bytes - b1 == first_update
    dev.update_positions(_tensor(posB), reclip=True)     # the device path: the reduction's scratch
    b2 = dev.device_bytes
    assert b2 - b1 == first_update + 4 * n_used + 7 * 8 * 256
    dev.update_positions(_tensor(posB), reclip=True)
    dev.update_positions(posB)
    assert dev.device_bytes == b2
    dev.close()
    twin.close()


# ---- reserve_cus ----
def test_device_tensor_update_between_two_frames_on_the_cu_masked_stream():
    import torch

    key = ("gen", "cornell")
    hs, posB = pc.case(key)
    dev = _scene(hs, "sah", reserve_cus=32)
    twin = rtamd.DeviceScene(hs, 0, tree="sah")
    p = _params(hs, key)
    outs = [torch.zeros((p.camera.height, p.camera.width, 3), dtype=torch.float64, device="cuda:0") for _ in range(2)]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = _tensor(hs.soa_arrays()["vertex_pos"])
        t += _tensor(posB - hs.soa_arrays()["vertex_pos"])     # made on the caller's stream
    want_pos = t.cpu().numpy()
    dev.launch(p, outs[0].data_ptr(), stream=stream.cuda_stream)
    dev.update_positions(t, stream=stream.cuda_stream)
    dev.launch(p, outs[1].data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    got = [o.cpu().numpy() for o in outs]
    assert np.array_equal(pc.bits(got[0]), pc.bits(twin.render(p)[0]))
    hs.update_vertices(want_pos)
    twin.update(hs)
    assert np.array_equal(pc.bits(got[1]), pc.bits(twin.render(p)[0]))
    assert _same_images(_images(dev), _images(twin))
    assert not np.array_equal(got[0], got[1])
    dev.close()
    twin.close()


# ---- canonical counters ----
def test_canonical_counters_are_refused_after_update_positions():
    key = ("gen", "cornell")
    hs, posB = pc.case(key)
    dev = _scene(hs, None)
    p = _params(hs, key, flags=rtamd.RT_FLAG_TRAVERSAL_STATS)
    _, st = dev.render(p)
    assert st.node_visits > 0 and st.tri_tests > 0
    dev.update_positions(posB)
    img = np.zeros((p.camera.height, p.camera.width, 3))
    st = abi.Stats()
    lib = rtamd.hip_lib()
    assert lib.rt_render_to_host(dev._h, C.byref(p), img.ctypes.data_as(C.c_void_p), C.byref(st)) == abi.RT_ERR_UNSUPPORTED
    assert b"RT_FLAG_TRAVERSAL_STATS" in lib.rt_last_error()
    _, wide = dev.render(_params(hs, key, flags=rtamd.RT_FLAG_WIDE_STATS))
    assert wide.node_visits > 0 and wide.tri_tests > 0
    dev.close()
