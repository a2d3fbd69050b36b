"""rt_trace_radiance without a GPU: symbol, binding, argument checks, DeviceScene.radiance's input
checks, and the pure-numpy helpers panorama_rays / tile_major."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import rtamd
from rtamd import abi

import radiance_cases as rc


def test_radiance_symbol_exported_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", str(rtamd.HIP_LIB)], capture_output=True, text=True,
                         check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert "rt_trace_radiance" in names
    assert "rt_trace_radiance" in abi.HIP_SYMBOLS
    header = (rtamd.HIP_LIB.parents[2] / "include" / "rt_hip.h").read_text()
    assert "int rt_trace_radiance(" in header and "RT_RADIANCE_MAX_RAYS" in header
    fn = rtamd.hip_lib().rt_trace_radiance
    assert fn.restype is C.c_int and len(fn.argtypes) == 7


def _good_params():
    hs, _ = rc.scene("cornell")
    return rc.params(hs, 8, 8)


def test_radiance_rejects_bad_arguments_before_any_hip_call():
    # no GPU here: a non-null scene pointer is never dereferenced before the checks
    lib = rtamd.hip_lib()
    buf = (C.c_double * 8)()
    ptr = C.cast(buf, C.c_void_p)
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    p = _good_params()
    P = C.byref(p)
    bad_args = [
        (None, P, ptr, 1, ptr, None, None),          # null scene
        (None, P, ptr, 0, ptr, None, None),          # ... also with no rays
        (fake, None, ptr, 1, ptr, None, None),       # null params
        (fake, P, ptr, -1, ptr, None, None),         # negative count
        (fake, P, None, 1, ptr, None, None),         # null rays
        (fake, P, ptr, 1, None, None, None),         # null results
        (fake, P, ptr, (1 << 31) + 1, ptr, None, None),   # past RT_RADIANCE_MAX_RAYS
    ]
    for args in bad_args:
        assert lib.rt_trace_radiance(*args) == abi.RT_ERR_INVALID, args
        assert lib.rt_last_error()
    flags = [abi.RT_FLAG_TRAVERSAL_STATS, abi.RT_FLAG_WIDE_STATS, abi.RT_FLAG_TIMELINE, abi.RT_FLAG_TILE_COST,
             abi.RT_FLAG_TILE_COST_TIME, abi.RT_FLAG_COST_ORDER, abi.RT_FLAG_GLOBAL_ROWS,
             abi.RT_FLAG_NATURAL_ORDER | abi.RT_FLAG_COST_ORDER, 1 << 20]
    bad_fields = [{"spp_n": 2}, {"spp_n": 0}, {"row_begin": 1}, {"row_end": 4}, {"stripe_count": 2},
                  {"stripe_count": 2, "stripe_index": 1}, {"stripe_index": 1}, {"out_format": 2}, {"out_format": -1}]
    bad_fields += [{"flags": f} for f in flags]
    for fields in bad_fields:
        q = rc.copy_params(p, **fields)
        for n in (1, 0):   # checked whatever the count
            assert lib.rt_trace_radiance(fake, C.byref(q), ptr, n, ptr, None, None) == abi.RT_ERR_INVALID, fields
            assert lib.rt_last_error()


def test_radiance_of_no_rays_is_ok_without_a_device():
    # n == 0 with valid arguments returns before any HIP call, buffers may be null, stats are zeroed
    lib = rtamd.hip_lib()
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    p = _good_params()
    for flags in (0, abi.RT_FLAG_NATURAL_ORDER):
        q = rc.copy_params(p, flags=flags)
        st = abi.Stats(primary_rays=-1, pixels=-1)
        assert lib.rt_trace_radiance(fake, C.byref(q), None, 0, None, C.byref(st), None) == abi.RT_OK
        assert (st.primary_rays, st.shadow_rays, st.reflection_rays, st.pixels) == (0, 0, 0, 0)


def test_radiance_method_checks_its_rays_before_calling_the_library():
    import torch

    dev = object.__new__(rtamd.DeviceScene)   # no upload: the checks come first
    dev.device = 0
    dev._h = None
    p = _good_params()
    for rays in (np.zeros((4, 7)), np.zeros(8), np.zeros((2, 4, 8)),            # shape
                 torch.zeros((4, 8), dtype=torch.float32),                      # dtype
                 torch.zeros((4, 8), dtype=torch.float64),                      # device (a CPU tensor)
                 torch.zeros((4, 7), dtype=torch.float64),
                 torch.zeros((8, 8), dtype=torch.float64)[::2],                 # not contiguous
                 [[0.0] * 8]):
        with pytest.raises(ValueError):
            dev.radiance(rays, p)


def test_radiance_method_reports_a_library_without_the_symbol(monkeypatch):
    class Partial:   # what abi.bind(..., partial=True) leaves of a library built from an older source
        def __getattr__(self, name):
            raise AttributeError(name)

    p = _good_params()
    dev = object.__new__(rtamd.DeviceScene)
    dev.device = 0
    dev._h = None
    monkeypatch.setattr(rtamd, "hip_lib", lambda: Partial())
    with pytest.raises(rtamd.RtError) as e:
        dev.radiance(np.zeros((1, 8)), p)
    assert type(e.value) is rtamd.RtError and "rt_trace_radiance" in str(e.value)


def test_panorama_rays_shape_order_and_directions():
    hs, _ = rc.scene("office")
    p = hs.render_params(96, 54, 1)
    W, H = 32, 16
    rays = rtamd.panorama_rays(p, W, H)
    assert rays.shape == (H * W, 8) and rays.dtype == np.float64
    assert np.all(rays[:, 6] == np.inf) and np.all(rays[:, 7] == 0.0)
    assert np.array_equal(rays[:, 0:3], np.tile(np.array(p.camera.eye[:]), (H * W, 1)))
    d = rays[:, 3:6].reshape(H, W, 3)
    assert np.abs(np.sqrt((d * d).sum(-1)) - 1.0).max() <= 1e-15
    cam = p.camera
    eye, ll = np.array(cam.eye[:]), np.array(cam.lower_left[:])
    xd, yd = np.array(cam.x_dir[:]), np.array(cam.y_dir[:])
    fwd = ll + 0.5 * cam.width * xd + 0.5 * cam.height * yd - eye
    right, up, fwd = xd / np.linalg.norm(xd), yd / np.linalg.norm(yd), fwd / np.linalg.norm(fwd)
    # the pixel nearest the centre points along forward: half a pixel off in phi and in theta
    centre = d[H // 2, W // 2]
    assert np.dot(centre, fwd) >= np.cos(np.pi / W) * np.cos(0.5 * np.pi / H) - 1e-15
    assert np.dot(centre, fwd) == max(np.dot(v, fwd) for v in d.reshape(-1, 3))
    # row 0 is the bottom row: within pi / (2 H) of -up, the top row of +up
    lim = np.cos(0.5 * np.pi / H) - 1e-15
    assert np.all(d[0] @ -up >= lim) and np.all(d[H - 1] @ up >= lim)
    # pixel (x, y) by the formula, row-major
    x, y = 5, 11
    phi, theta = 2 * np.pi * (x + 0.5) / W - np.pi, np.pi * (y + 0.5) / H - 0.5 * np.pi
    want = np.cos(theta) * np.sin(phi) * right + np.sin(theta) * up + np.cos(theta) * np.cos(phi) * fwd
    assert np.abs(rays[y * W + x, 3:6] - want).max() <= 1e-15
    # columns x and x + W / 2 mirror each other in the horizontal plane: the same height, the
    # opposite horizontal part
    a, b = d[:, : W // 2], d[:, W // 2:]
    assert np.abs(a @ up - b @ up).max() <= 1e-15
    ha, hb = a - (a @ up)[..., None] * up, b - (b @ up)[..., None] * up
    assert np.abs(ha + hb).max() <= 1e-15


@pytest.mark.parametrize("w,h", [(64, 48), (70, 50), (8, 8), (5, 3), (9, 17)])
def test_tile_major_is_the_tile_order_permutation(w, h):
    tw, th = rtamd.tile_shape()
    assert (tw, th) == (8, 8)
    perm = rtamd.tile_major(w, h)
    assert perm.shape == (w * h,) and np.array_equal(np.sort(perm), np.arange(w * h))
    ys, xs = perm // w, perm % w
    # the first entries are the pixels of tile (0, 0)
    n0 = min(w, tw) * min(h, th)
    assert {(int(x), int(y)) for x, y in zip(xs[:n0], ys[:n0])} == {(x, y) for y in range(min(h, th))
                                                                    for x in range(min(w, tw))}
    # tiles in row-major order, each tile's pixels consecutive (partial edge tiles included)
    tile = (ys // th) * (-(-w // tw)) + xs // tw
    assert np.all(np.diff(tile) >= 0)
    sizes = np.bincount(tile)
    assert sizes.max() == min(w, tw) * min(h, th) and sizes.sum() == w * h
    if w % tw and h % th:
        assert sizes[-1] == (w % tw) * (h % th)   # the top-right corner tile
    inv = np.argsort(perm)
    assert np.array_equal(np.arange(w * h)[perm][inv], np.arange(w * h))
