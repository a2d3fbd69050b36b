"""The vertex-update C ABI without a GPU: symbols, rt_scene_update's layout, the
argument checks of rt_scene_update_vertices, rt_debug_scene_image and rt_host_update_vertices that
need no scene, and rt_refit.hpp's outward rounding in a stand-alone program under UBSan / ASan
against nextafterf."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import rtamd
from rtamd import abi

ROOT = Path(__file__).resolve().parents[1]
HIP = {"rt_scene_update_vertices": 3, "rt_debug_scene_image": 4}
HOST = {"rt_host_update_vertices": 3}


def _exported(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib_path)], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split()}


def test_update_symbols_exported_declared_and_bound():
    for path, lib, table, header, syms in (
            (rtamd.HIP_LIB, rtamd.hip_lib(), abi.HIP_SYMBOLS, "rt_hip.h", HIP),
            (rtamd.HOST_LIB, rtamd.host_lib(), abi.HOST_SYMBOLS, "rt_host.h", HOST)):
        names = _exported(path)
        text = (ROOT / "include" / header).read_text()
        for sym, nargs in syms.items():
            assert sym in names, sym
            assert sym in table, sym
            assert f" {sym}(" in text, sym
            assert len(getattr(lib, sym).argtypes) == nargs, sym
    header = (ROOT / "include" / "rt_hip.h").read_text()
    assert "enum { RT_IMAGE_NODES4 = 0, RT_IMAGE_TRIS = 1, RT_IMAGE_TNORM = 2 };" in header
    assert (abi.RT_IMAGE_NODES4, abi.RT_IMAGE_TRIS, abi.RT_IMAGE_TNORM) == (0, 1, 2)
    for method in ("update", "update_vertices", "debug_scene_image"):
        assert callable(getattr(rtamd.DeviceScene, method))
    assert callable(rtamd.HostScene.update_vertices)


def test_scene_update_layout_matches_c(tmp_path):
    fields = ["n_vertices", "n_triangles", "vertex_pos", "vertex_normals", "face_normals", "reserved_"]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rt_hip.h"', "int main(void){",
           'printf("%zu\\n", sizeof(rt_scene_update));']
    src += [f'printf("%zu\\n", offsetof(rt_scene_update, {f}));' for f in fields]
    src.append("return 0;}")
    (tmp_path / "upd_sizes.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-o", str(tmp_path / "upd_sizes"), str(tmp_path / "upd_sizes.c")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "upd_sizes")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got[0] == C.sizeof(abi.SceneUpdate) == 64
    assert got[1:] == [getattr(abi.SceneUpdate, f).offset for f in fields]


def _update(pos=True, vn=True, fn=True):
    a = np.zeros((4, 3))
    dp = C.POINTER(C.c_double)
    u = abi.SceneUpdate(n_vertices=4, n_triangles=4, vertex_pos=a.ctypes.data_as(dp) if pos else None,
                        vertex_normals=a.ctypes.data_as(dp) if vn else None,
                        face_normals=a.ctypes.data_as(dp) if fn else None)
    u._keep = a
    return u


def test_update_rejects_null_arguments():
    # checked before any HIP call and before the scene is read: no GPU needed, the non-null scene
    # pointer is never dereferenced
    lib = rtamd.hip_lib()
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    cases = [((None, C.byref(_update()), None), b"null argument"), ((fake, None, None), b"null argument"),
             ((fake, C.byref(_update(pos=False)), None), b"null array"),
             ((fake, C.byref(_update(vn=False)), None), b"null array"),
             ((fake, C.byref(_update(fn=False)), None), b"null array")]
    for args, why in cases:
        assert lib.rt_tile_shape(None, None) == abi.RT_ERR_INVALID   # another call's message in between
        assert lib.rt_scene_update_vertices(*args) == abi.RT_ERR_INVALID
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_scene_update_vertices:") and why in msg, msg
    buf = (C.c_char * 16)()
    assert lib.rt_debug_scene_image(None, abi.RT_IMAGE_NODES4, buf, 16) == abi.RT_ERR_INVALID
    assert lib.rt_debug_scene_image(fake, abi.RT_IMAGE_NODES4, None, 16) == abi.RT_ERR_INVALID
    assert lib.rt_debug_scene_image(fake, abi.RT_IMAGE_NODES4, buf, -1) == abi.RT_ERR_INVALID
    assert lib.rt_debug_scene_image(fake, 3, buf, 16) == abi.RT_ERR_INVALID
    assert lib.rt_debug_scene_image(fake, -1, buf, 16) == abi.RT_ERR_INVALID


def test_host_update_errors():
    lib = rtamd.host_lib()
    a = np.zeros((4, 3))
    dp = a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.rt_host_update_vertices(None, dp, 4) == abi.RT_ERR_INVALID
    hs = rtamd.HostScene.generate("cornell")
    assert lib.rt_host_update_vertices(hs.handle, dp, 4) == abi.RT_ERR_INVALID   # not prepared
    assert b"not prepared" in lib.rt_host_last_error()
    hs.prepare()
    n = hs.soa.contents.n_vertices
    assert lib.rt_host_update_vertices(hs.handle, None, n) == abi.RT_ERR_INVALID
    for bad in (0, n - 1, n + 1, -1):
        assert lib.rt_host_update_vertices(hs.handle, dp, bad) == abi.RT_ERR_INVALID
        assert b"n_vertices" in lib.rt_host_last_error()


ROUND_PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "%s/my-raytracer_amd/csrc/device/rt_refit.hpp"
static int check(double x) {
  float f = (float)x, g = (float)x;
  if ((double)f > x) f = std::nextafterf(f, -INFINITY);
  if ((double)g < x) g = std::nextafterf(g, INFINITY);
  const float a = rt_refit_round_down(x), b = rt_refit_round_up(x);
  return std::memcmp(&a, &f, 4) != 0 || std::memcmp(&b, &g, 4) != 0 || !((double)a <= x) || !((double)b >= x);
}
int main() {
  long long bad = 0, n = 0;
  uint64_t s = 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < 2000000; ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    double x;
    std::memcpy(&x, &s, 8);
    if (x != x) continue;
    bad += check(x); ++n;
    const double y = std::ldexp((double)(s >> 11) / 9007199254740992.0 - 0.5, (int)(s %% 300) - 170);
    bad += check(y); ++n;
  }
  const double edge[] = {0.0, -0.0, 1e-46, -1e-46, 1e-45, -1e-45, 3.4028234e38, 3.5e38, -3.5e38, 1e300, -1e300,
                         INFINITY, -INFINITY, 1.17549435e-38, -1.17549435e-38, 1.1754942e-38, 1.0, -1.0,
                         1.0 + 1e-10, -1.0 - 1e-10, 16777217.0, -16777217.0};
  for (double x : edge) { bad += check(x); ++n; }
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const double p[3] = {NAN, 1.0, -2.0}, q[3] = {3.0, NAN, 5.0};
  rt_refit_grow(lo, hi, p);
  rt_refit_grow(lo, hi, q);
  bad += !(lo[0] == 3.0 && hi[0] == 3.0 && lo[1] == 1.0 && hi[1] == 1.0 && lo[2] == -2.0 && hi[2] == 5.0);
  const float l4[4] = {1.f, INFINITY, -2.f, INFINITY}, h4[4] = {2.f, -INFINITY, 7.f, -INFINITY};
  float l, h;
  rt_refit_union4(l4, h4, &l, &h);
  bad += !(l == -2.f && h == 7.f);
  std::printf("%%lld %%lld\n", n, bad);
  return 0;
}
"""


def test_refit_header_under_sanitizers(tmp_path):
    (tmp_path / "round.cpp").write_text(ROUND_PROGRAM % ROOT)
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(tmp_path / "round"), str(tmp_path / "round.cpp")], check=True)
    out = subprocess.run([str(tmp_path / "round")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) > 3_000_000 and int(out[1]) == 0, out
