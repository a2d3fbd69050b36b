"""Camera C ABI without a GPU: symbols, rt_camera_out's layout, the argument checks of
rt_trace_camera, rt_camera_rays_host and rt_surface_points_host, both host functions against their
numpy restatement (camera_cases) bit for bit, and the header under UBSan / ASan in a stand-alone
program on the same inputs."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rtamd
from rtamd import abi

import camera_cases as cc
import query_cases as qc

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = {"rt_trace_camera": 5, "rt_camera_rays_host": 3, "rt_surface_points_host": 5}


def _host():
    return qc.scene("cornell")[0]


def test_camera_symbols_exported_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", str(rtamd.HIP_LIB)], capture_output=True, text=True,
                         check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    header = (ROOT / "include" / "rt_hip.h").read_text()
    lib = rtamd.hip_lib()
    for sym, nargs in SYMBOLS.items():
        assert sym in names, sym
        assert sym in abi.HIP_SYMBOLS, sym
        assert f" {sym}(" in header, sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym
    assert "enum { RT_CAMERA_ROW_MAJOR = 0, RT_CAMERA_TILE_MAJOR = 1 };" in header
    assert "#define RT_CAMERA_MAX_PIXELS (1LL << 31)" in header
    assert (abi.RT_CAMERA_ROW_MAJOR, abi.RT_CAMERA_TILE_MAJOR, abi.RT_CAMERA_MAX_PIXELS) == (0, 1, 1 << 31)


def test_camera_out_layout_matches_c(tmp_path):
    fields = ["d_hits", "d_points", "order", "reserved_", "point_tmax"]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rt_hip.h"', "int main(void){",
           'printf("%zu\\n", sizeof(rt_camera_out));']
    src += [f'printf("%zu\\n", offsetof(rt_camera_out, {f}));' for f in fields]
    src.append("return 0;}")
    (tmp_path / "cam_sizes.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-o", str(tmp_path / "cam_sizes"), str(tmp_path / "cam_sizes.c")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "cam_sizes")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got[0] == C.sizeof(abi.CameraOut)
    assert got[1:] == [getattr(abi.CameraOut, f).offset for f in fields]


def _clear_error(lib):
    """Leaves another call's message in rt_last_error, so that a stale one cannot pass for a new one."""
    assert lib.rt_tile_shape(None, None) == abi.RT_ERR_INVALID
    assert lib.rt_last_error().startswith(b"rt_tile_shape:")


def _bad_params(hs):
    """(params, why): everything the camera entry points refuse about rt_render_params."""
    def make(W=32, H=24, **kw):
        p = hs.render_params(32, 24, 1)
        p.camera.width, p.camera.height = W, H
        p.row_begin, p.row_end = 0, 0   # every row of the camera, whatever its height
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    return [(make(spp_n=2), b"spp_n"), (make(spp_n=0), b"spp_n"),
            (make(flags=abi.RT_FLAG_GLOBAL_ROWS), b"RT_FLAG_NATURAL_ORDER"),
            (make(flags=abi.RT_FLAG_COST_ORDER), b"RT_FLAG_NATURAL_ORDER"),
            (make(flags=abi.RT_FLAG_NATURAL_ORDER | abi.RT_FLAG_TRAVERSAL_STATS), b"RT_FLAG_NATURAL_ORDER"),
            (make(W=0), b"bad image size"), (make(H=0), b"bad image size"), (make(W=-4), b"bad image size"),
            (make(W=65536, H=4), b"bad image size"), (make(W=4, H=65536), b"bad image size"),
            (make(stripe_count=2, stripe_index=2), b"stripe_index"), (make(stripe_index=-1), b"stripe_index"),
            (make(stripe_index=1), b"stripe_index"),
            (make(**cc.SHARD_REFUSED), b"row ranges cannot be combined"),
            (make(stripe_count=2, row_begin=3), b"row ranges cannot be combined"),
            # 2^32 pixels: the pixel limit speaks before the per-side one
            (make(W=65536, H=65536), b"RT_CAMERA_MAX_PIXELS"),
            (make(W=65535, H=65535), b"RT_CAMERA_MAX_PIXELS")]


def _out(hits=True, points=False, order=abi.RT_CAMERA_ROW_MAJOR, point_tmax=float("inf")):
    buf = (C.c_char * 256)()
    o = abi.CameraOut(d_hits=C.addressof(buf) if hits else None, d_points=C.addressof(buf) if points else None,
                      order=order, point_tmax=point_tmax)
    o._keep = buf
    return o


def test_trace_camera_rejects_bad_arguments():
    # checked before any HIP call: no GPU needed.  The non-null scene pointer is never dereferenced.
    lib = rtamd.hip_lib()
    hs = _host()
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    ok, out = hs.render_params(32, 24, 1), _out()
    cases = [((None, C.byref(ok), C.byref(out), None, None), b"null scene"),
             ((fake, None, C.byref(out), None, None), b"null parameters"),
             ((fake, C.byref(ok), None, None, None), b"null output"),
             ((fake, C.byref(ok), C.byref(_out(hits=False)), None, None), b"neither hits nor points"),
             ((fake, C.byref(ok), C.byref(_out(order=2)), None, None), b"unknown order"),
             ((fake, C.byref(ok), C.byref(_out(order=-1)), None, None), b"unknown order")]
    for tmax in (float("nan"), 0.0, 1e-5, -1.0, float("-inf")):
        cases.append(((fake, C.byref(ok), C.byref(_out(points=True, point_tmax=tmax)), None, None), b"point_tmax"))
        cases.append(((fake, C.byref(ok), C.byref(_out(hits=False, points=True, point_tmax=tmax)), None, None),
                      b"point_tmax"))
    keep = _bad_params(hs)
    for p, why in keep:
        cases.append(((fake, C.byref(p), C.byref(out), None, None), why))
    for args, why in cases:
        _clear_error(lib)
        assert lib.rt_trace_camera(*args) == abi.RT_ERR_INVALID, why
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_trace_camera:") and why in msg, (why, msg)


def test_point_tmax_is_not_checked_without_points():
    # an empty row range passes every check and returns before the scene is touched: RT_OK shows
    # that nothing before that point refused the arguments
    lib = rtamd.hip_lib()
    hs = _host()
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    p = cc.params(hs, 32, 24, row_begin=7, row_end=7)
    assert rtamd.rows_in_shard(p) == 0
    for tmax in (float("nan"), 0.0, 1e-5):
        _clear_error(lib)
        assert lib.rt_trace_camera(fake, C.byref(p), C.byref(_out(point_tmax=tmax)), None, None) == abi.RT_OK
        assert lib.rt_trace_camera(fake, C.byref(p), C.byref(_out(points=True, point_tmax=tmax)), None,
                                   None) == abi.RT_ERR_INVALID
        assert b"point_tmax" in lib.rt_last_error()
    for tmax in (1.0000001e-5, 2.5, float("inf")):
        assert lib.rt_trace_camera(fake, C.byref(p), C.byref(_out(points=True, point_tmax=tmax)), None, None) == abi.RT_OK
    p.flags = abi.RT_FLAG_NATURAL_ORDER   # accepted, changes nothing
    assert lib.rt_trace_camera(fake, C.byref(p), C.byref(_out()), None, None) == abi.RT_OK


def test_host_functions_reject_bad_arguments():
    lib = rtamd.hip_lib()
    hs = _host()
    buf = (C.c_char * (64 * 32 * 24))()
    ptr = C.c_void_p(C.addressof(buf))
    ok = hs.render_params(32, 24, 1)
    cases = [((None, 0, ptr), b"null parameters"), ((C.byref(ok), 2, ptr), b"unknown order"),
             ((C.byref(ok), -1, ptr), b"unknown order"), ((C.byref(ok), 0, None), b"null ray buffer")]
    keep = _bad_params(hs)
    cases += [((C.byref(p), 0, ptr), why) for p, why in keep]
    for args, why in cases:
        _clear_error(lib)
        assert lib.rt_camera_rays_host(*args) == abi.RT_ERR_INVALID, why
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_camera_rays_host:") and why in msg, (why, msg)
    inf = float("inf")
    cases = [((ptr, ptr, -1, inf, ptr), b"negative record count"),
             ((ptr, ptr, (1 << 31) + 1, inf, ptr), b"RT_CAMERA_MAX_PIXELS"),
             ((None, ptr, 1, inf, ptr), b"null ray, hit or point"), ((ptr, None, 1, inf, ptr), b"null ray, hit or point"),
             ((ptr, ptr, 1, inf, None), b"null ray, hit or point")]
    cases += [((ptr, ptr, 1, t, ptr), b"point_tmax") for t in (float("nan"), 0.0, 1e-5, -2.0)]
    cases += [((None, None, 0, float("nan"), None), b"point_tmax")]
    for args, why in cases:
        _clear_error(lib)
        assert lib.rt_surface_points_host(*args) == abi.RT_ERR_INVALID, why
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_surface_points_host:") and why in msg, (why, msg)
    # n = 0: nothing to do, whatever the pointers
    assert lib.rt_surface_points_host(None, None, 0, inf, None) == abi.RT_OK
    assert rtamd.surface_points_host(np.zeros((0, 8)), np.zeros((0, 8))).shape == (0, 8)
    empty = cc.params(hs, 32, 24, row_begin=7, row_end=7)
    assert lib.rt_camera_rays_host(C.byref(empty), 0, None) == abi.RT_OK
    assert rtamd.camera_rays_host(empty, "tile").shape == (0, 8)


@pytest.mark.parametrize("order", cc.ORDERS)
@pytest.mark.parametrize("W,H", cc.CAMERAS)
def test_camera_rays_host_equals_numpy(W, H, order):
    p = cc.params(_host(), W, H)
    got = rtamd.camera_rays_host(p, order)
    want = cc.numpy_rays(p, order)
    assert got.shape == (W * H, 8) and cc.same_bits(got, want)
    assert np.all(got[:, 6] == np.inf) and np.all(got[:, 7] == 0.0)
    if order == "row":
        assert cc.same_bits(got, rtamd.camera_rays(p))


@pytest.mark.parametrize("order", cc.ORDERS)
@pytest.mark.parametrize("shard", sorted(cc.SHARDS))
def test_camera_rays_host_shards(shard, order):
    hs = _host()
    p = cc.params(hs, 32, 24, **cc.SHARDS[shard])
    ys = cc.shard_rows(p)
    assert len(ys) == rtamd.rows_in_shard(p) and 0 < len(ys)
    got = rtamd.camera_rays_host(p, order)
    assert got.shape == (len(ys) * 32, 8) and cc.same_bits(got, cc.numpy_rays(p, order))
    # the shard's rays are the full frame's rays of its rows
    full = rtamd.camera_rays(hs.render_params(32, 24, 1)).reshape(24, 32, 8)[ys].reshape(-1, 8)
    if order == "tile":
        full = full[rtamd.tile_major(32, len(ys))]
    assert cc.same_bits(got, full)
    if shard != "full":
        assert len(ys) == 12 and len(ys) % 8 != 0   # a partial tile row at the top
    if shard == "range_sh3":
        assert ys[0] == 5 and ys[0] % 3 != 0
    if shard.startswith("stripe"):
        assert ys[:4] == ([0, 1, 2, 6] if shard == "stripe0" else [3, 4, 5, 9])


def test_tile_order_differs_from_row_order_and_keeps_every_pixel():
    p = cc.params(_host(), 13, 11)
    row, tile = rtamd.camera_rays_host(p, "row"), rtamd.camera_rays_host(p, "tile")
    assert not cc.same_bits(row, tile)
    key = lambda r: sorted(map(bytes, np.ascontiguousarray(r)))   # noqa: E731
    assert key(row) == key(tile) and len(set(key(row))) == 13 * 11


@pytest.mark.parametrize("point_tmax", [np.inf, 2.5])
def test_surface_points_host_equals_numpy(point_tmax):
    rays, hits = cc.synthetic()
    got = rtamd.surface_points_host(rays, hits, point_tmax)
    want = cc.numpy_points(rays, hits, point_tmax)
    assert got.shape == rays.shape and cc.same_bits(got, want)
    assert np.all(got[:, 6] == point_tmax) and np.all(got[:, 7] == 0.0)
    # the ground this claims to cover is in the inputs
    miss = ~(hits[:, 0] < np.inf)
    flip = cc.flipped(rays, hits)
    assert miss.sum() > 100 and flip.sum() > 100 and (~flip & ~miss).sum() > 100
    assert cc.same_bits(got[miss, 0:3], rays[miss, 0:3]) and np.all(got[miss, 3:6] == 0.0)
    assert not np.any(np.signbit(got[miss, 3:6]))
    assert cc.same_bits(got[flip, 3:6], -hits[flip, 3:6])
    assert cc.same_bits(got[~flip & ~miss, 3:6], hits[~flip & ~miss, 3:6])
    d, n = rays[0:16, 3:6], hits[0:16, 3:6]
    assert np.all((n * d).sum(1) == 0.0) and not flip[0:16].any()       # a dot product of exactly 0
    assert np.all(got[16:28, 3:6] == 0.0) and np.all(np.signbit(got[24:28, 3:6]))   # zero normals keep their sign
    ln = np.sqrt((rays[36:60, 3:6] ** 2).sum(1))
    assert np.all(ln[:12] < 1e-149) and np.all(ln[12:] > 1e149)
    assert np.all(np.isfinite(got[36:60, 0:3]))
    # |p - o| = t along the normalised direction
    t = hits[36:60, 0]
    assert np.max(np.abs(np.sqrt(((got[36:60, 0:3] - rays[36:60, 0:3]) ** 2).sum(1)) / t - 1.0)) < 1e-12


SANITIZED_MAIN = r"""
#include "rt_camera_point.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
static std::vector<double> slurp(const char* path) {
  std::vector<double> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) std::exit(4);
  double x;
  while (std::fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}
static int dump(const char* path, const std::vector<double>& v) {
  FILE* f = std::fopen(path, "wb");
  if (!f || std::fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) return 7;
  std::fclose(f);
  return 0;
}
// argv: camera (12 doubles) W H, rays.bin hits.bin point_tmax, out_rays.bin out_points.bin
int main(int argc, char** argv) {
  if (argc != 9) return 5;
  const std::vector<double> cam = slurp(argv[1]);
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
  if (cam.size() != 12) return 6;
  std::vector<double> rays((size_t)W * H * 8, 0.0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      double* r = &rays[((size_t)y * W + x) * 8];
      rt_camera_ray(&cam[0], &cam[3], &cam[6], &cam[9], x, y, r, r + 3);
      r[6] = INFINITY;
    }
  const std::vector<double> in_rays = slurp(argv[4]), in_hits = slurp(argv[5]);
  const double point_tmax = std::atof(argv[6]);
  const size_t n = in_rays.size() / 8;
  if (in_hits.size() != in_rays.size()) return 6;
  std::vector<double> pts(n * 8, 0.0);
  unsigned long long misses = 0;
  for (size_t i = 0; i < n; ++i) {
    const double* r = &in_rays[i * 8];
    const double* h = &in_hits[i * 8];
    double* p = &pts[i * 8];
    rt_surface_point(r, r + 3, h[0], h + 3, p, p + 3);
    p[6] = point_tmax;
    if (!(h[0] < INFINITY)) ++misses;
  }
  if (dump(argv[7], rays) || dump(argv[8], pts)) return 7;
  std::printf("%d x %d rays, %zu points, %llu misses\n", W, H, n, misses);
  return 0;
}
"""


def test_camera_header_is_clean_under_sanitizers(tmp_path):
    # a stand-alone program (its own main, no preloaded runtime) over the inputs of the numpy tests
    p = cc.params(_host(), 13, 11)
    cam = p.camera
    np.array(cam.eye[:] + cam.lower_left[:] + cam.x_dir[:] + cam.y_dir[:]).tofile(tmp_path / "cam.bin")
    rays, hits = cc.synthetic()
    rays.tofile(tmp_path / "rays.bin")
    hits.tofile(tmp_path / "hits.bin")
    (tmp_path / "cam_main.cpp").write_text(SANITIZED_MAIN)
    exe = tmp_path / "cam_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover", "-I", str(ROOT / "my-raytracer_amd" / "csrc" / "device"),
                    "-o", str(exe), str(tmp_path / "cam_main.cpp")], check=True, timeout=300)
    run = subprocess.run([str(exe), str(tmp_path / "cam.bin"), "13", "11", str(tmp_path / "rays.bin"),
                          str(tmp_path / "hits.bin"), "2.5", str(tmp_path / "out_rays.bin"),
                          str(tmp_path / "out_pts.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    misses = int((~(hits[:, 0] < np.inf)).sum())
    assert f"13 x 11 rays, {len(rays)} points, {misses} misses" in run.stdout
    assert cc.same_bits(np.fromfile(tmp_path / "out_rays.bin").reshape(-1, 8), rtamd.camera_rays_host(p, "row"))
    assert cc.same_bits(np.fromfile(tmp_path / "out_pts.bin").reshape(-1, 8), rtamd.surface_points_host(rays, hits, 2.5))


def test_python_layer_checks_its_inputs():
    p = cc.params(_host(), 13, 11)
    with pytest.raises(ValueError):
        rtamd.camera_rays_host(p, "morton")
    with pytest.raises(ValueError):
        rtamd.surface_points_host(np.zeros((4, 7)), np.zeros((4, 7)))
    with pytest.raises(ValueError):
        rtamd.surface_points_host(np.zeros((4, 8)), np.zeros((3, 8)))
    with pytest.raises(rtamd.RtError):
        rtamd.surface_points_host(np.zeros((4, 8)), np.zeros((4, 8)), point_tmax=0.0)
    p.spp_n = 2
    with pytest.raises(rtamd.RtError):
        rtamd.camera_rays_host(p)
    # DeviceScene.camera refuses before it touches a device
    dev = object.__new__(rtamd.DeviceScene)
    dev.device = 0
    dev._h = None
    q = cc.params(_host(), 13, 11)
    with pytest.raises(ValueError):
        dev.camera(q, order="morton")
    with pytest.raises(ValueError):
        dev.camera(q, hits=False, points=False)


def test_python_layer_reports_a_library_without_the_symbols(monkeypatch):
    class Partial:   # what abi.bind(..., partial=True) leaves of a library built from an older source
        def __getattr__(self, name):
            raise AttributeError(name)

    dev = object.__new__(rtamd.DeviceScene)
    dev.device = 0
    dev._h = None
    p = cc.params(_host(), 13, 11)
    monkeypatch.setattr(rtamd, "hip_lib", lambda: Partial())
    for call, sym in ((lambda: dev.camera(p), "rt_trace_camera"),
                      (lambda: rtamd.camera_rays_host(p), "rt_camera_rays_host"),
                      (lambda: rtamd.surface_points_host(np.zeros((1, 8)), np.zeros((1, 8))), "rt_surface_points_host")):
        with pytest.raises(rtamd.RtError) as e:
            call()
        assert type(e.value) is rtamd.RtError and sym in str(e.value)
