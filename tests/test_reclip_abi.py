"""The re-clipping update's C ABI without a GPU: symbols, the flag constant, the
argument checks of rt_scene_update_vertices_ex and the host helpers that need no scene, and
tools/reclip_check.cpp -- the new kernel body run on build_image's SceneImage by a stand-alone
program under ASan / UBSan."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import reclip_cases as rcs
import rtamd
from rtamd import abi

ROOT = Path(__file__).resolve().parents[1]
AMD = ROOT / "my-raytracer_amd"
HIP = {"rt_scene_update_vertices_ex": 4, "rt_debug_clip_regions": 6, "rt_reclip_box_host": 6}


def test_reclip_symbols_exported_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", str(rtamd.HIP_LIB)], capture_output=True, text=True,
                         check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    text = (ROOT / "include" / "rt_hip.h").read_text()
    for sym, nargs in HIP.items():
        assert sym in names and sym in abi.HIP_SYMBOLS and f" {sym}(" in text, sym
        assert len(getattr(rtamd.hip_lib(), sym).argtypes) == nargs, sym
    assert "enum { RT_UPDATE_RECLIP = 1 };" in text
    assert abi.RT_UPDATE_RECLIP == 1
    assert "rt_scene_update_vertices" in names   # the plain call stays
    assert callable(rtamd.clip_regions) and callable(rtamd.reclip_box_host)
    import inspect
    for method in (rtamd.DeviceScene.update, rtamd.DeviceScene.update_vertices):
        assert inspect.signature(method).parameters["reclip"].default is False


def _update():
    a = np.zeros((4, 3))
    dp = C.POINTER(C.c_double)
    u = abi.SceneUpdate(n_vertices=4, n_triangles=4, vertex_pos=a.ctypes.data_as(dp),
                        vertex_normals=a.ctypes.data_as(dp), face_normals=a.ctypes.data_as(dp))
    u._keep = a
    return u


def test_update_ex_rejects_bad_arguments_before_any_hip_call():
    # no GPU needed: the non-null scene pointer is never dereferenced
    lib = rtamd.hip_lib()
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    u = _update()
    for flags in (0, abi.RT_UPDATE_RECLIP):
        assert lib.rt_tile_shape(None, None) == abi.RT_ERR_INVALID   # another call's message in between
        assert lib.rt_scene_update_vertices_ex(None, C.byref(u), flags, None) == abi.RT_ERR_INVALID
        assert b"null argument" in lib.rt_last_error()
        assert lib.rt_scene_update_vertices_ex(fake, None, flags, None) == abi.RT_ERR_INVALID
    for flags in (2, 3, 4, 0x80000000, 0xfffffffe):
        assert lib.rt_tile_shape(None, None) == abi.RT_ERR_INVALID
        assert lib.rt_scene_update_vertices_ex(fake, C.byref(u), flags, None) == abi.RT_ERR_INVALID
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_scene_update_vertices:") and b"unknown flag" in msg, msg


def test_host_helpers_reject_bad_arguments():
    lib = rtamd.hip_lib()
    hs = rcs.host_a(rcs.PLAIN_SEED)
    opt = rtamd.upload_options()
    clip, slot = np.zeros(6), np.zeros(1, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert lib.rt_debug_clip_regions(hs.soa, hs.bvh, C.byref(opt), clip.ctypes.data_as(dp), slot.ctypes.data_as(ip), -1) \
        == abi.RT_ERR_INVALID
    assert lib.rt_debug_clip_regions(hs.soa, hs.bvh, C.byref(opt), None, slot.ctypes.data_as(ip), 1) == abi.RT_ERR_INVALID
    assert lib.rt_debug_clip_regions(hs.soa, hs.bvh, C.byref(opt), clip.ctypes.data_as(dp), None, 1) == abi.RT_ERR_INVALID
    # a short buffer gets the first rows only; NULL options are the defaults
    n = lib.rt_debug_clip_regions(hs.soa, hs.bvh, None, clip.ctypes.data_as(dp), slot.ctypes.data_as(ip), 1)
    assert n == rcs.RECORDS[rcs.PLAIN_SEED][0] and 0 <= slot[0] < n
    p = np.zeros(3).ctypes.data_as(dp)
    c6 = np.zeros(6).ctypes.data_as(dp)
    for missing in range(6):
        args = [p, p, p, c6, p, p]
        args[missing] = None
        assert lib.rt_reclip_box_host(*args) == abi.RT_ERR_INVALID


def test_reclip_kernel_body_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.fail("hipcc not found: the stand-alone check of the kernel body needs it")
    exe = tmp_path / "reclip_check"
    image_o = AMD / "lib" / "device_image.o"
    if not image_o.exists():   # (a tree that carries the libraries without their object files)
        image_o = tmp_path / "device_image.o"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-c", "-o", str(image_o),
                        str(AMD / "csrc" / "host" / "device_image.cpp")], check=True)
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'include'}", f"-I{AMD / 'csrc'}", str(ROOT / "tools" / "reclip_check.cpp"),
                    f"-Wl,{image_o}",f"-L{AMD / 'lib'}", "-lrt_host", f"-Wl,-rpath,{AMD / 'lib'}",
                    "-lpthread", "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 4 and all(ln.endswith("ok") for ln in lines)
