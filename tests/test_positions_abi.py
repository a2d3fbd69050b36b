"""The positions-update C ABI without a GPU: symbols, rt_scene_positions' layout, the
argument checks of rt_scene_set_triangle_order and rt_scene_update_positions that need no device, and
tools/normals_check.cpp -- the kernel bodies against HostMesh::compute_normals in a stand-alone
program under ASan / UBSan.

The checks that read the scene run on a zeroed block standing in for an rt_scene: a scene without
triangles, vertices, order tables or watchdog word.  They come before any HIP call and read plain
integer and pointer members only, so no device is needed; a scene without triangles needs no
device for rt_scene_set_triangle_order either."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rtamd
from rtamd import abi

ROOT = Path(__file__).resolve().parents[1]
AMD = ROOT / "my-raytracer_amd"
HIP = {"rt_scene_set_triangle_order": 3, "rt_scene_update_positions": 4, "rt_normals_host": 7}
HOST = {"rt_host_slot_triangles": 1}


def _exported(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib_path)], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split()}


def test_positions_symbols_exported_declared_and_bound():
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
    for method in ("set_triangle_order", "update_positions"):
        assert callable(getattr(rtamd.DeviceScene, method))
    assert callable(rtamd.HostScene.slot_triangles)
    mk = (AMD / "Makefile").read_text()
    assert "csrc/device/rt_normals.hpp" in mk and "csrc/device/rt_normals.inc" in mk


def test_scene_positions_layout_matches_c(tmp_path):
    fields = ["n_vertices", "vertex_pos", "on_device", "reserved_", "reserved2_"]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rt_hip.h"', "int main(void){",
           'printf("%zu\\n", sizeof(rt_scene_positions));']
    src += [f'printf("%zu\\n", offsetof(rt_scene_positions, {f}));' for f in fields]
    src.append("return 0;}")
    (tmp_path / "pos_sizes.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-o", str(tmp_path / "pos_sizes"), str(tmp_path / "pos_sizes.c")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "pos_sizes")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got[0] == C.sizeof(abi.ScenePositions) == 48
    assert got[1:] == [getattr(abi.ScenePositions, f).offset for f in fields]


def _positions(n=4, ptr=True, on_device=0):
    a = np.zeros((max(n, 1), 3))
    p = abi.ScenePositions(n_vertices=n, vertex_pos=a.ctypes.data if ptr else None, on_device=on_device)
    p._keep = a
    return p


def _empty_scene():
    """A zeroed block in place of an rt_scene (see the module docstring)."""
    block = (C.c_char * (4 << 20))()
    return block, C.cast(block, C.c_void_p)


def test_update_positions_rejects_bad_arguments():
    lib = rtamd.hip_lib()
    _block, sc = _empty_scene()
    cases = [((None, C.byref(_positions()), 0, None), b"null argument"),
             ((sc, None, 0, None), b"null argument"),
             ((sc, C.byref(_positions(ptr=False)), 0, None), b"null array"),
             ((sc, C.byref(_positions(0)), 2, None), b"unknown flag"),
             ((sc, C.byref(_positions(0)), abi.RT_UPDATE_RECLIP | 4, None), b"unknown flag"),
             ((sc, C.byref(_positions(0, on_device=2)), 0, None), b"on_device"),
             ((sc, C.byref(_positions(4)), 0, None), b"n_vertices"),
             ((sc, C.byref(_positions(-1)), abi.RT_UPDATE_RECLIP, None), b"n_vertices"),
             # the counts and flags are right, but the scene has had no rt_scene_set_triangle_order call
             ((sc, C.byref(_positions(0)), 0, None), b"rt_scene_set_triangle_order"),
             ((sc, C.byref(_positions(0, on_device=1)), abi.RT_UPDATE_RECLIP, None), b"rt_scene_set_triangle_order")]
    for args, why in cases:
        assert lib.rt_tile_shape(None, None) == abi.RT_ERR_INVALID   # another call's message in between
        assert lib.rt_scene_update_positions(*args) == abi.RT_ERR_INVALID, why
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_scene_update_positions:") and why in msg, msg


def test_set_triangle_order_rejects_bad_arguments():
    lib = rtamd.hip_lib()
    _block, sc = _empty_scene()
    ip = C.POINTER(C.c_int)
    perm = np.array([2, 0, 1, 3], dtype=np.int32)
    cases = [((None, perm.ctypes.data_as(ip), 4), abi.RT_ERR_INVALID, b"null argument"),
             ((sc, None, 4), abi.RT_ERR_INVALID, b"null argument"),
             ((sc, perm.ctypes.data_as(ip), -1), abi.RT_ERR_INVALID, b"negative"),
             ((sc, perm.ctypes.data_as(ip), (1 << 31) // 3 + 1), abi.RT_ERR_UNSUPPORTED, b"32-bit"),
             ((sc, perm.ctypes.data_as(ip), 4), abi.RT_ERR_INVALID, b"differs from the uploaded scene's")]
    for bad in ([0, 1, 1, 3], [0, 1, 2, 4], [0, -1, 2, 3], [3, 3, 3, 3]):
        arr = np.array(bad, dtype=np.int32)
        perm_case = ((sc, arr.ctypes.data_as(ip), 4), abi.RT_ERR_INVALID, b"not a permutation")
        cases.append(perm_case + (arr,))
    for case in cases:
        args, code, why = case[:3]
        assert lib.rt_tile_shape(None, None) == abi.RT_ERR_INVALID
        assert lib.rt_scene_set_triangle_order(*args) == code, why
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_scene_set_triangle_order:") and why in msg, msg


def test_scene_without_triangles_needs_no_launch():
    # the order of nothing is accepted without a HIP call; afterwards an update of no vertices is
    # RT_OK without a launch, from a host and from a (never read) device pointer
    lib = rtamd.hip_lib()
    _block, sc = _empty_scene()
    none = np.zeros(1, dtype=np.int32)
    assert lib.rt_scene_update_positions(sc, C.byref(_positions(0)), 0, None) == abi.RT_ERR_INVALID
    assert lib.rt_scene_set_triangle_order(sc, none.ctypes.data_as(C.POINTER(C.c_int)), 0) == abi.RT_OK
    assert lib.rt_scene_device_bytes(sc) == 0
    for on_device in (0, 1):
        assert lib.rt_scene_update_positions(sc, C.byref(_positions(0, on_device=on_device)), 0, None) == abi.RT_OK
    assert lib.rt_scene_update_positions(sc, C.byref(_positions(1)), 0, None) == abi.RT_ERR_INVALID
    # replacing the (empty) tables releases the first ones
    assert lib.rt_scene_set_triangle_order(sc, none.ctypes.data_as(C.POINTER(C.c_int)), 0) == abi.RT_OK
    assert lib.rt_scene_device_bytes(sc) == 0


def test_python_wrappers_reject_bad_shapes():
    hs = rtamd.HostScene.generate("cornell")
    with pytest.raises(rtamd.RtError, match="not prepared"):
        hs.slot_triangles()
    dev = object.__new__(rtamd.DeviceScene)   # no device: the shape checks come first
    dev._h, dev.device = C.c_void_p(), 0
    with pytest.raises(ValueError):
        dev.update_positions(np.zeros((4, 2)))
    with pytest.raises(ValueError):
        dev.update_positions(np.zeros(12))
    with pytest.raises(ValueError):
        dev.set_triangle_order(np.zeros((2, 2), dtype=np.int32))
    import torch
    for bad in (torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float32)):
        with pytest.raises(ValueError):       # a CPU tensor: another device
            dev.update_positions(bad)


def test_normal_kernel_bodies_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.fail("hipcc not found: the stand-alone check of the kernel bodies needs it")
    exe = tmp_path / "normals_check"
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'include'}", f"-I{AMD / 'csrc'}", str(ROOT / "tools" / "normals_check.cpp"),
                    f"-L{AMD / 'lib'}", "-lrt_host", f"-Wl,-rpath,{AMD / 'lib'}", "-lpthread", "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 7 and all(ln.endswith("ok") for ln in lines)
    assert sum("normals ==" in ln for ln in lines) == 6 and sum("bounds ==" in ln for ln in lines) == 4
