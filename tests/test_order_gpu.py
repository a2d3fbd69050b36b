"""rt_ray_order / rt_permute_rows and trace / radiance with an order on the GPU.
Every expectation is numpy's (order_cases.numpy_keys, np.argsort(kind="stable"), fancy indexing) or
the unchanged entry points' own result (order=None), compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import rtamd
from rtamd import abi

import order_cases as oc
import query_cases as qc
import radiance_cases as rc

pytestmark = pytest.mark.gpu

T = abi.RT_ORDER_TILE
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]
PATTERN = 0x5A


def _scene(name):
    return qc.scene(name, qc.SCENES[name].get("n_triangles", 0))


_dev = {}


def _device(name):
    """One upload per scene, shared by the tests of this module."""
    if name not in _dev:
        _dev[name] = rtamd.DeviceScene(_scene(name)[0], 0)
    return _dev[name]


_mixed = {}


def _mixed_rays(name):
    """random_rays mixed with vertex_rays, the latter quantised in origin so that many keys repeat;
    6 * T rays in a fixed shuffle.  Computed once, not modified."""
    if name not in _mixed:
        hs, _, P, _, _ = _scene(name)
        a = qc.random_rays(hs, n=3 * T, seed=7)
        b = qc.vertex_rays(hs, P, n=3 * T, seed=5)
        b[:, 0:3] = b[0, 0:3]                    # one origin: keys differ by direction only
        b[T:, 3:6] = b[:2 * T, 3:6]              # and every direction twice or more
        rays = np.concatenate([a, b])
        _mixed[name] = rays[np.random.default_rng(1).permutation(len(rays))]
    return _mixed[name]


def _order_buffers(n, slack=64):
    """Over-allocated, pattern-filled (perm, keys, work) byte tensors for rt_ray_order of n rays."""
    import torch

    wb = rtamd.order_workspace_bytes(n)
    perm = torch.full((4 * (n + slack),), PATTERN, dtype=torch.uint8, device="cuda")
    keys = torch.full((4 * (n + slack),), PATTERN, dtype=torch.uint8, device="cuda")
    work = torch.full((wb + 4096,), PATTERN, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    return perm, keys, work


def _order_launch(dev, d_rays, n, ob, buffers, want_keys=True, stream=None):
    """rt_ray_order into buffers that are ready; synchronises nothing."""
    perm, keys, work = buffers
    rc_ = rtamd.hip_lib().rt_ray_order(dev._h, C.c_void_p(d_rays.data_ptr()), n, ob, C.c_void_p(perm.data_ptr()),
                                       C.c_void_p(keys.data_ptr()) if want_keys else None,
                                       C.c_void_p(work.data_ptr()), C.c_void_p(stream) if stream else None)
    assert rc_ == abi.RT_OK, rtamd.hip_lib().rt_last_error()


def _order_raw(dev, d_rays, n, ob, want_keys=True):
    """rt_ray_order on the null stream into fresh pattern-filled buffers -> (perm, keys, work)."""
    import torch

    buffers = _order_buffers(n)
    torch.cuda.synchronize()
    _order_launch(dev, d_rays, n, ob, buffers, want_keys)
    return buffers


def _check_order(dev, rays, n, ob, grid=0):
    import torch

    lo, hi = dev.bounds()
    want_keys = oc.numpy_keys(lo, hi, rays[:n], ob)
    d_rays = torch.from_numpy(rays[:n].copy()).cuda()
    assert rtamd.hip_lib().rt_debug_set_order_grid(dev._h, grid) == abi.RT_OK
    try:
        perm, keys, work = _order_raw(dev, d_rays, n, ob)
        torch.cuda.synchronize()
    finally:
        rtamd.hip_lib().rt_debug_set_order_grid(dev._h, 0)
    perm, keys, work = perm.cpu().numpy(), keys.cpu().numpy(), work.cpu().numpy()
    assert np.array_equal(keys[:4 * n].view(np.uint32), want_keys)
    assert np.array_equal(perm[:4 * n].view(np.uint32), np.argsort(want_keys, kind="stable").astype(np.uint32))
    # guards: nothing at or past n entries, or past the workspace's bytes, changed
    assert np.all(perm[4 * n:] == PATTERN) and np.all(keys[4 * n:] == PATTERN)
    assert np.all(work[rtamd.order_workspace_bytes(n):] == PATTERN)


def test_bounds_are_the_root_box_widened(gpu_available):
    hs = _scene("cornell")[0]
    lo, hi = _device("cornell").bounds()
    rlo, rhi = qc.root_box(hs)
    assert np.all(lo <= rlo) and np.all(hi >= rhi) and np.all(hi > lo)
    # the layout's delta is 2^-20 of the scene's size
    slack = 1e-5 * (np.abs(np.concatenate([rlo, rhi])).max() + (rhi - rlo).max())
    assert np.all(rlo - lo <= slack) and np.all(hi - rhi <= slack)


@pytest.mark.parametrize("ob", [0, -1, 10])
@pytest.mark.parametrize("name", ["cornell", "random_tris"])
def test_order_is_numpys_stable_argsort_of_the_numpy_keys(gpu_available, name, ob):
    dev, rays = _device(name), _mixed_rays(name)
    for n in SIZES:
        _check_order(dev, rays, n, ob)


@pytest.mark.parametrize("ob", [0, -1, 10])
def test_blocks_that_own_several_tiles(gpu_available, ob):
    # two blocks: the first owns three tiles, the second two whole ones and a partial one
    _check_order(_device("cornell"), _mixed_rays("cornell"), 5 * T + 3, ob, grid=2)
    _check_order(_device("cornell"), _mixed_rays("cornell"), 5 * T + 3, ob, grid=1)


def test_stability_and_degenerate_rays(gpu_available):
    dev = _device("cornell")
    hs = _scene("cornell")[0]
    good = qc.random_rays(hs, n=1000, seed=3)
    same = np.tile(good[:1], (1000, 1))
    perm = dev.ray_order(same)
    assert perm.dtype == np.uint32 and np.array_equal(perm, np.arange(1000))
    bad = np.tile(oc.degenerate_rays(), (30, 1))
    perm, keys = dev.ray_order(bad, keys=True)
    assert np.all(keys == abi.RT_ORDER_KEY_DEGENERATE) and np.array_equal(perm, np.arange(len(bad)))
    # degenerate rays among valid ones come last, in index order
    mix = good.copy()
    where = np.random.default_rng(9).choice(1000, 137, replace=False)
    mix[where] = np.resize(oc.degenerate_rays(), (137, 8))
    perm, keys = dev.ray_order(mix, keys=True)
    assert np.array_equal(perm[-137:], np.sort(where))
    assert np.all(keys[perm[:-137]] < (1 << 31)) and np.all(np.diff(keys[perm].astype(np.int64)) >= 0)
    lo, hi = dev.bounds()
    assert np.array_equal(perm, np.argsort(oc.numpy_keys(lo, hi, mix), kind="stable"))


def test_order_without_keys_and_tensor_plumbing(gpu_available):
    import torch

    dev, rays = _device("cornell"), _mixed_rays("cornell")[:2 * T + 5]
    lo, hi = dev.bounds()
    want = np.argsort(oc.numpy_keys(lo, hi, rays, 3), kind="stable")
    d_rays = torch.from_numpy(rays).cuda()
    perm, _, _ = _order_raw(dev, d_rays, len(rays), 3, want_keys=False)
    torch.cuda.synchronize()
    assert np.array_equal(perm.cpu().numpy()[:4 * len(rays)].view(np.uint32), want)
    got = dev.ray_order(d_rays, origin_bits=3)
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    got, keys = dev.ray_order(d_rays, origin_bits=3, keys=True, stream=torch.cuda.Stream().cuda_stream)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), oc.numpy_keys(lo, hi, rays, 3))


@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("row_bytes", [1, 4, 12, 24, 64])
def test_permute_rows_gathers_and_scatters_like_numpy(gpu_available, row_bytes, n):
    import torch

    rng = np.random.default_rng(row_bytes * 1000 + n)
    src = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
    perm = rng.permutation(n).astype(np.int32)
    shape = {1: (torch.uint8, (n,)), 4: (torch.float32, (n,)), 12: (torch.float32, (n, 3)),
             24: (torch.float64, (n, 3)), 64: (torch.float64, (n, 8))}[row_bytes]
    d_src = torch.from_numpy(src).cuda().view(shape[0]).reshape(shape[1]).contiguous()
    d_perm = torch.from_numpy(perm).cuda()

    def bytes_of(t):
        return t.cpu().contiguous().view(torch.uint8).numpy().reshape(n, row_bytes)

    gathered = rtamd.permute_rows(d_src, d_perm)
    assert gathered.dtype == d_src.dtype and gathered.shape == d_src.shape
    assert np.array_equal(bytes_of(gathered), src[perm])
    scattered = rtamd.permute_rows(d_src, d_perm, inverse=True)
    want = np.zeros_like(src)
    want[perm] = src
    assert np.array_equal(bytes_of(scattered), want)
    back = rtamd.permute_rows(gathered, d_perm, inverse=True, stream=torch.cuda.Stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(bytes_of(back), src)


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("row_bytes", [1, 12, 64])
def test_permute_rows_skips_entries_out_of_range(gpu_available, row_bytes, inverse):
    # buffers of n + 1 rows whose last row is a pattern: a missing check shows as a changed or a
    # copied pattern, not as an access outside an allocation
    import torch

    n = 65
    rng = np.random.default_rng(5)
    src = rng.integers(0, 200, (n + 1, row_bytes), dtype=np.uint8)
    src[n] = 0xEE
    perm = rng.permutation(n).astype(np.uint32)
    skipped = [0, 17, 64]
    perm[skipped] = n
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((n + 1, row_bytes), 0xDD, dtype=torch.uint8, device="cuda")
    d_perm = torch.from_numpy(perm.view(np.int32)).cuda()
    assert rtamd.hip_lib().rt_permute_rows(C.c_void_p(d_src.data_ptr()), C.c_void_p(d_dst.data_ptr()),
                                           C.c_void_p(d_perm.data_ptr()), n, row_bytes, inverse, 0, None) == abi.RT_OK
    torch.cuda.synchronize()
    want = np.full((n + 1, row_bytes), 0xDD, dtype=np.uint8)
    keep = np.array([j for j in range(n) if j not in skipped])
    if inverse:
        want[perm[keep]] = src[keep]
    else:
        want[keep] = src[perm[keep]]
    assert np.array_equal(d_dst.cpu().numpy(), want)
    assert np.array_equal(d_src.cpu().numpy(), src)


@pytest.mark.parametrize("name", ["cornell", "office"])
def test_trace_with_an_order_returns_the_same_bits(gpu_available, name):
    import torch

    hs = _scene(name)[0]
    dev = _device(name)
    rays = qc.random_rays(hs)
    plain, st0 = dev.trace(rays, stats=True)
    occ0, so0 = dev.trace(rays, occluded=True, stats=True)
    assert 0 < st0.hits < 4096
    mine = np.random.default_rng(2).permutation(4096)
    for order in ("auto", dev.ray_order(rays, origin_bits=0), mine):
        got, st = dev.trace(rays, stats=True, order=order)
        assert sorted(got) == sorted(plain)
        for k in plain:
            assert got[k].dtype == plain[k].dtype and got[k].tobytes() == plain[k].tobytes(), k
        assert (st.rays, st.hits) == (st0.rays, st0.hits) == (4096, st0.hits)
        occ, so = dev.trace(rays, occluded=True, stats=True, order=order)
        assert occ.dtype == np.uint8 and np.array_equal(occ, occ0)
        assert (so.rays, so.hits) == (so0.rays, so0.hits)
    # tensors in, tensors out, on a stream
    d_rays = torch.from_numpy(rays).cuda()
    got = dev.trace(d_rays, order="auto", stream=torch.cuda.Stream().cuda_stream)
    torch.cuda.synchronize()
    for k in plain:
        assert got[k].is_cuda and got[k].cpu().numpy().tobytes() == plain[k].tobytes(), k


@pytest.mark.parametrize("fmt", [rtamd.RT_OUT_RGB_F64, rtamd.RT_OUT_RGB_F32])
@pytest.mark.parametrize("name", ["cornell", "office"])
def test_radiance_with_an_order_returns_the_same_bits(gpu_available, name, fmt):
    hs = _scene(name)[0]
    dev = _device(name)
    p = rc.params(hs, 64, 48, fmt)
    rays = rtamd.camera_rays(p)
    rays = rays[np.random.default_rng(4).permutation(len(rays))]
    plain, st0 = dev.radiance(rays, p, stats=True)
    assert rc.counts(st0)[0] == 64 * 48 and rc.counts(st0)[1] > 0
    perm = dev.ray_order(rays)
    for order in ("auto", perm):
        got, st = dev.radiance(rays, p, stats=True, order=order)
        assert got.dtype == plain.dtype and got.shape == plain.shape and got.tobytes() == plain.tobytes()
        assert rc.counts(st) == rc.counts(st0)
    # the same order serves a trace of the same rays
    assert dev.trace(rays, order=perm)["t"].tobytes() == dev.trace(rays)["t"].tobytes()
    got = dev.radiance(rays[:65], p, order="auto")
    assert got.tobytes() == plain[:65].tobytes()


def test_two_orders_beside_a_render_on_three_streams(gpu_available):
    import torch

    hs = _scene("office")[0]
    dev = _device("office")
    lo, hi = dev.bounds()
    rays_a, rays_b = qc.random_rays(hs, n=4 * T + 9, seed=21), qc.random_rays(hs, n=3 * T + 1, seed=22)
    d_a, d_b = torch.from_numpy(rays_a).cuda(), torch.from_numpy(rays_b).cuda()
    p = hs.render_params(96, 54, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    serial = torch.zeros((20, 54, 96, 3), dtype=torch.float64, device="cuda")
    dev.launch_frames(p, [serial[f].data_ptr() for f in range(20)])
    torch.cuda.synchronize()
    frames = torch.zeros_like(serial)
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    # every buffer made and filled first; then the three launches back to back, nothing waited for
    buf_a, buf_b = _order_buffers(len(rays_a)), _order_buffers(len(rays_b))
    torch.cuda.synchronize()
    dev.launch_frames(p, [frames[f].data_ptr() for f in range(20)], stream=s3.cuda_stream)
    _order_launch(dev, d_a, len(rays_a), -1, buf_a, stream=s1.cuda_stream)
    _order_launch(dev, d_b, len(rays_b), 0, buf_b, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    (pa, ka, wa), (pb, kb, wb) = buf_a, buf_b
    for perm, keys, work, rays, ob in ((pa, ka, wa, rays_a, -1), (pb, kb, wb, rays_b, 0)):
        n, want_keys = len(rays), oc.numpy_keys(lo, hi, rays, ob)
        assert np.array_equal(keys.cpu().numpy()[:4 * n].view(np.uint32), want_keys)
        assert np.array_equal(perm.cpu().numpy()[:4 * n].view(np.uint32), np.argsort(want_keys, kind="stable"))
        assert bool((perm[4 * n:] == PATTERN).all()) and bool((work[rtamd.order_workspace_bytes(n):] == PATTERN).all())
    assert bool((frames == serial).all())
    assert dev.status() == abi.RT_OK


def test_zero_rays_launch_nothing(gpu_available):
    import torch

    dev = _device("cornell")
    lib = rtamd.hip_lib()
    buf = torch.full((1024,), PATTERN, dtype=torch.uint8, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert lib.rt_ray_order(dev._h, p, 0, -1, p, p, p, None) == abi.RT_OK
    assert lib.rt_ray_order(dev._h, None, 0, -1, None, None, None, None) == abi.RT_OK
    odd = C.c_void_p(buf.data_ptr() + 3)   # unused at n = 0: its alignment does not matter
    assert lib.rt_ray_order(dev._h, p, 0, -1, p, None, odd, None) == abi.RT_OK
    torch.cuda.synchronize()
    assert bool((buf == PATTERN).all())
    perm, keys = dev.ray_order(np.zeros((0, 8)), keys=True)
    assert perm.shape == (0,) and keys.shape == (0,)
    empty = torch.zeros((0, 8), dtype=torch.float64, device="cuda")
    assert rtamd.permute_rows(empty, torch.zeros((0,), dtype=torch.int32, device="cuda")).shape == (0, 8)
    assert dev.trace(np.zeros((0, 8)), order="auto")["t"].shape == (0,)
