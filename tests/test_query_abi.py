"""Ray-query C ABI without a GPU: symbols, struct layouts, argument checks, camera_rays."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import pyoracle
import rtamd
from rtamd import abi

import query_cases

ROOT = Path(__file__).resolve().parents[1]


def test_query_symbols_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", str(rtamd.HIP_LIB)], capture_output=True, text=True,
                         check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    lib = rtamd.hip_lib()
    for sym in ("rt_trace_closest", "rt_trace_occluded"):
        assert sym in names
        assert sym in abi.HIP_SYMBOLS
        fn = getattr(lib, sym)
        assert fn.restype is C.c_int and len(fn.argtypes) == 6


def test_query_struct_layouts_match_c(tmp_path):
    structs = {"rt_ray": abi.Ray, "rt_hit": abi.Hit, "rt_query_stats": abi.QueryStats}
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rt_hip.h"', "int main(void){"]
    for name in structs:
        src.append(f'printf("{name} %zu\\n", sizeof({name}));')
    for field in ("slot", "mesh", "prim", "normal"):
        src.append(f'printf("hit.{field} %zu\\n", offsetof(rt_hit, {field}));')
    src.append('printf("ray.tmax %zu\\n", offsetof(rt_ray, tmax));')
    src.append("return 0;}")
    (tmp_path / "sizes.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-o", str(tmp_path / "sizes"), str(tmp_path / "sizes.c")], check=True)
    out = subprocess.run([str(tmp_path / "sizes")], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    for name, cls in structs.items():
        assert got[name] == 64 and C.sizeof(cls) == 64, name
    # the [n, 8] float64 views of DeviceScene.trace: ints at words 12, 13, 14 of a row
    assert (got["hit.slot"], got["hit.mesh"], got["hit.prim"]) == (48, 52, 56)
    assert (abi.Hit.slot.offset, abi.Hit.mesh.offset, abi.Hit.prim.offset) == (48, 52, 56)
    assert got["hit.normal"] == abi.Hit.normal.offset == 24
    assert got["ray.tmax"] == abi.Ray.tmax.offset == 48


def test_query_entry_points_reject_bad_arguments():
    # checked before any HIP call: no GPU needed.  A non-null scene pointer is never dereferenced
    # before the buffer checks.
    lib = rtamd.hip_lib()
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    for fn in (lib.rt_trace_closest, lib.rt_trace_occluded):
        for args in ((None, p, 1, p, None, None),       # null scene
                     (None, p, 0, p, None, None),
                     (fake, p, -1, p, None, None),      # negative count
                     (fake, None, 1, p, None, None),    # null rays
                     (fake, p, 1, None, None, None)):   # null results
            assert fn(*args) == abi.RT_ERR_INVALID, args
            assert lib.rt_last_error()


def test_camera_rays_reproduce_the_oracles_primary_hits():
    hs, orc, _, _, _ = query_cases.scene("cornell")
    p = hs.render_params(5, 3, 1)
    rays = rtamd.camera_rays(p)
    assert rays.shape == (15, 8) and rays.dtype == np.float64
    assert np.all(rays[:, 6] == np.inf) and np.all(rays[:, 7] == 0.0)
    assert np.array_equal(rays[:, 0:3], np.tile(np.array(p.camera.eye[:]), (15, 1)))
    xy = np.array([(x, y) for y in range(3) for x in range(5)], dtype=np.int32)   # row-major, row 0 first
    pix, _ = orc.render_pixels(p, xy)
    lit = np.any(pix != np.array(p.background[:]), axis=1)
    hit = np.array([orc.closest_hit(r[0:3], r[3:6]) is not None for r in rays])
    assert hit.any() and np.array_equal(hit, lit)
    # the direction in the oracle's order: ((lower_left + x * x_dir) + y * y_dir) - eye
    cam = p.camera
    x, y = 3, 2
    want = [(cam.lower_left[k] + x * cam.x_dir[k]) + y * cam.y_dir[k] - cam.eye[k] for k in range(3)]
    assert list(rays[y * 5 + x, 3:6]) == want
