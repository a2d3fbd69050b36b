"""Ray-order C ABI without a GPU: symbols, argument checks, the workspace formula,
the coherence key against its numpy restatement (order_cases.numpy_keys), the key header under
UBSan / ASan in a stand-alone program, and the coherence the key's definition buys."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rtamd
from rtamd import abi

import order_cases

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = {"rt_scene_bounds": 3, "rt_ray_order_workspace_bytes": 1, "rt_ray_keys_host": 6, "rt_ray_order": 8,
           "rt_permute_rows": 8, "rt_debug_set_order_grid": 2}
LO, HI = np.array([-1.0, 0.0, 2.0]), np.array([3.0, 0.5, 10.0])


def test_order_symbols_exported_declared_and_bound():
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
    assert lib.rt_ray_order_workspace_bytes.restype is C.c_size_t
    for macro, value in (("RT_ORDER_MAX_RAYS", "(1LL << 31)"), ("RT_ORDER_KEY_DEGENERATE", "0x80000000u"),
                         ("RT_ORDER_TILE", str(abi.RT_ORDER_TILE))):
        assert f"#define {macro} {value}" in header
    assert abi.RT_ORDER_MAX_RAYS == 1 << 31 and abi.RT_ORDER_KEY_DEGENERATE == 0x80000000


def _clear_error(lib):
    """Leaves another call's message in rt_last_error, so that a stale one cannot pass for a new one."""
    assert lib.rt_tile_shape(None, None) == abi.RT_ERR_INVALID
    assert lib.rt_last_error().startswith(b"rt_tile_shape:")


def test_ray_order_rejects_bad_arguments():
    # checked before any HIP call: no GPU needed.  A non-null scene pointer is never dereferenced
    # before the buffer checks.
    lib = rtamd.hip_lib()
    buf = (C.c_char * 1024)()
    p = C.c_void_p((C.addressof(buf) + 255) // 256 * 256)
    odd = C.c_void_p(p.value + 64)
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    for args, why in (((None, p, 1, -1, p, None, p, None), b"null scene"),
                      ((None, p, 0, -1, p, None, p, None), b"null scene"),
                      ((fake, p, -1, -1, p, None, p, None), b"negative ray count"),
                      ((fake, p, (1 << 31) + 1, -1, p, None, p, None), b"RT_ORDER_MAX_RAYS"),
                      ((fake, None, 1, -1, p, None, p, None), b"null ray, permutation or workspace"),
                      ((fake, p, 1, -1, None, None, p, None), b"null ray, permutation or workspace"),
                      ((fake, p, 1, -1, p, None, None, None), b"null ray, permutation or workspace"),
                      ((fake, p, 1, -2, p, None, p, None), b"origin_bits"),
                      ((fake, p, 1, 11, p, None, p, None), b"origin_bits"),
                      ((fake, p, 1, -1, p, None, odd, None), b"256-byte aligned")):
        _clear_error(lib)
        assert lib.rt_ray_order(*args) == abi.RT_ERR_INVALID, args
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_ray_order:") and why in msg, (args, msg)
    three = (C.c_double * 3)()
    for fn, args in ((lib.rt_debug_set_order_grid, (None, 2)), (lib.rt_debug_set_order_grid, (fake, -1)),
                     (lib.rt_scene_bounds, (None, three, three)), (lib.rt_scene_bounds, (fake, None, three))):
        _clear_error(lib)
        assert fn(*args) == abi.RT_ERR_INVALID, args
        assert lib.rt_last_error().startswith(fn.__name__.encode() + b":")


def test_permute_rows_rejects_bad_arguments_and_accepts_no_rows():
    lib = rtamd.hip_lib()
    buf = (C.c_char * 4096)()
    a = (C.addressof(buf) + 255) // 256 * 256
    src, dst, perm = C.c_void_p(a), C.c_void_p(a + 2048), C.c_void_p(a + 1024)
    for args, why in (((src, dst, perm, -1, 64, 0, 0, None), b"negative row count"),
                      ((src, dst, perm, (1 << 32) + 1, 64, 0, 0, None), b"32-bit index"),
                      ((src, dst, perm, 4, 0, 0, 0, None), b"row_bytes"),
                      ((src, dst, perm, 4, 257, 0, 0, None), b"row_bytes"),
                      ((src, dst, perm, 4, -16, 1, 0, None), b"row_bytes"),
                      ((src, dst, perm, 4, 64, 0, -1, None), b"negative device"),
                      ((None, dst, perm, 4, 64, 0, 0, None), b"null buffer"),
                      ((src, None, perm, 4, 64, 1, 0, None), b"null buffer"),
                      ((src, dst, None, 4, 64, 0, 0, None), b"null buffer"),
                      ((C.c_void_p(a + 8), dst, perm, 4, 64, 0, 0, None), b"not aligned"),    # 64-B rows: 16 B
                      ((src, C.c_void_p(a + 2048 + 4), perm, 4, 24, 0, 0, None), b"not aligned"),   # 24-B rows: 8 B
                      ((src, C.c_void_p(a + 2048 + 2), perm, 4, 12, 1, 0, None), b"not aligned"),   # 12-B rows: 4 B
                      ((src, C.c_void_p(a + 1), perm, 4, 6, 0, 0, None), b"not aligned"),     # 6-B rows: 2 B
                      ((src, src, perm, 4, 64, 0, 0, None), b"overlap"),
                      ((src, C.c_void_p(a + 192), perm, 4, 64, 0, 0, None), b"overlap"),
                      ((C.c_void_p(a + 130), src, perm, 66, 2, 1, 0, None), b"overlap")):
        _clear_error(lib)
        assert lib.rt_permute_rows(*args) == abi.RT_ERR_INVALID, args
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_permute_rows:") and why in msg, (args, msg)
    # n = 0: nothing to do, no launch, whatever the pointers (null, unaligned, the same)
    assert lib.rt_permute_rows(None, None, None, 0, 64, 0, 0, None) == abi.RT_OK
    assert lib.rt_permute_rows(src, dst, perm, 0, 1, 1, 0, None) == abi.RT_OK
    assert lib.rt_permute_rows(C.c_void_p(a + 1), C.c_void_p(a + 1), perm, 0, 64, 0, 0, None) == abi.RT_OK


def test_ray_keys_host_rejects_bad_arguments_and_accepts_no_rays():
    lib = rtamd.hip_lib()
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1)
    rays = (C.c_double * 8)()
    keys = (C.c_uint * 1)()
    for args, why in (((None, hi, rays, 1, -1, keys), b"null box"), ((lo, None, rays, 1, -1, keys), b"null box"),
                      ((lo, hi, rays, -1, -1, keys), b"negative ray count"),
                      ((lo, hi, None, 1, -1, keys), b"null ray or key buffer"),
                      ((lo, hi, rays, 1, -1, None), b"null ray or key buffer"),
                      ((lo, hi, rays, 1, -2, keys), b"origin_bits"), ((lo, hi, rays, 1, 11, keys), b"origin_bits")):
        _clear_error(lib)
        assert lib.rt_ray_keys_host(*args) == abi.RT_ERR_INVALID, args
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_ray_keys_host:") and why in msg, (args, msg)
    assert lib.rt_ray_keys_host(lo, hi, None, 0, -1, None) == abi.RT_OK
    assert len(rtamd.ray_keys_host(LO, HI, np.zeros((0, 8)))) == 0


def test_python_layer_reports_a_library_without_the_symbols(monkeypatch):
    class Partial:   # what abi.bind(..., partial=True) leaves of a library built from an older source
        def __getattr__(self, name):
            raise AttributeError(name)

    dev = object.__new__(rtamd.DeviceScene)
    dev.device = 0
    dev._h = None
    monkeypatch.setattr(rtamd, "hip_lib", lambda: Partial())
    for call, sym in ((lambda: dev.ray_order(np.zeros((1, 8))), "rt_ray_order"),
                      (lambda: dev.bounds(), "rt_scene_bounds"),
                      (lambda: rtamd.permute_rows(None, None), "rt_permute_rows"),
                      (lambda: rtamd.order_workspace_bytes(1), "rt_ray_order_workspace_bytes"),
                      (lambda: rtamd.ray_keys_host(LO, HI, np.zeros((1, 8))), "rt_ray_keys_host")):
        with pytest.raises(rtamd.RtError) as e:
            call()
        assert type(e.value) is rtamd.RtError and sym in str(e.value)


def test_python_layer_checks_its_inputs():
    import torch

    with pytest.raises(ValueError):
        rtamd.permute_rows(torch.zeros((4, 8)), torch.zeros((4,), dtype=torch.int32))   # not a CUDA tensor
    with pytest.raises(ValueError):
        rtamd.ray_keys_host(LO, HI, np.zeros((4, 7)))


def test_workspace_bytes_follow_the_documented_formula():
    def formula(n):   # include/rt_hip.h
        return 3 * ((4 * n + 255) // 256 * 256) + 4 * 256 * 1024

    assert rtamd.order_workspace_bytes(0) == 0 and rtamd.order_workspace_bytes(-5) == 0
    for n in (1, 64, 65, 10 ** 6, 2 ** 31):
        assert rtamd.order_workspace_bytes(n) == formula(n), n
    sizes = [rtamd.order_workspace_bytes(n) for n in (0, 1, 2, 63, 64, 65, 1000, 1024, 1025, 10 ** 6, 2 ** 31)]
    assert sizes == sorted(sizes)


@pytest.fixture(scope="module")
def key_rays():
    """Every ray set the key is pinned on, as one array, in the box [LO, HI]."""
    sets = [order_cases.box_rays(LO, HI),
            order_cases.make_rays(0.5 * (LO + HI), order_cases.special_directions()),
            order_cases.extreme_rays(LO, HI),
            order_cases.degenerate_rays()]
    return np.concatenate(sets)


@pytest.mark.parametrize("ob", order_cases.ORIGIN_BITS)
def test_host_keys_equal_the_numpy_key(key_rays, ob):
    got = rtamd.ray_keys_host(LO, HI, key_rays, ob)
    want = order_cases.numpy_keys(LO, HI, key_rays, ob)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    nd = len(order_cases.degenerate_rays())
    assert np.all(got[-nd:] == abi.RT_ORDER_KEY_DEGENERATE)
    assert np.all(got[:-nd] < (1 << 31))
    # a box flat in one axis: that axis adds nothing
    hi_flat = HI.copy()
    hi_flat[1] = LO[1]
    assert np.array_equal(rtamd.ray_keys_host(LO, hi_flat, key_rays, ob),
                          order_cases.numpy_keys(LO, hi_flat, key_rays, ob))


def test_key_cells_at_the_edges():
    # origin on a hi face: the last cell; far outside: clamped; the layout of the default split
    mid = 0.5 * (LO + HI)
    rays = order_cases.make_rays([HI, LO, [1e300] * 3, [-1e300] * 3, mid], [0.0, 0.0, 1.0])
    keys = rtamd.ray_keys_host(LO, HI, rays, 5)
    md = int(keys[1])                         # origin cell 0: only the direction code
    assert md < (1 << 16)
    assert [int(k) >> 16 for k in keys] == [0x7fff, 0, 0x7fff, 0, 0b111 << 12]
    assert all(int(k) & 0xffff == md for k in keys)
    assert [order_cases.dir_bits(ob) for ob in (0, 5, 10)] == [15, 8, 0]
    # origin_bits = 10: no direction bits; 0: no origin bits
    assert int(rtamd.ray_keys_host(LO, HI, rays[:1], 10)[0]) == (1 << 30) - 1
    k0 = rtamd.ray_keys_host(LO, HI, rays, 0)
    assert len(set(int(k) for k in k0)) == 1 and int(k0[0]) < (1 << 30)


SANITIZED_MAIN = r"""
#include "rt_order_key.hpp"
#include <cstdio>
#include <limits>
int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double lo[3] = {-1.0, 0.0, 2.0}, hi[3] = {3.0, 0.5, 10.0}, flat[3] = {3.0, 0.0, 10.0};
  const double huge_lo[3] = {-1.7e308, -1.7e308, -1.7e308}, huge_hi[3] = {1.7e308, 1.7e308, 1.7e308};
  const double v[] = {0.0, -0.0, 1.0, -1.0, 0.5, 3.0, 10.0, 1e-310, -1e-310, 1e-150, 1e300, -1e300, 1.7e308, -1.7e308,
                      inf, -inf, nan};
  const int nv = sizeof v / sizeof v[0];
  const double tm[] = {inf, 1.0, 1e-5, 0.0, -1.0, nan};
  unsigned long long sum = 0, deg = 0, n = 0;
  for (int ob = -1; ob <= 10; ++ob)
    for (int a = 0; a < nv; ++a)
      for (int b = 0; b < nv; ++b)
        for (int c = 0; c < nv; ++c)
          for (int t = 0; t < 6; ++t) {
            const double p[3] = {v[a], v[b], v[c]}, q[3] = {v[c], v[a], v[b]};
            const double* los[3] = {lo, lo, huge_lo};
            const double* his[3] = {hi, flat, huge_hi};
            for (int box = 0; box < 3; ++box) {
              const uint32_t k = rt_order_key(los[box], his[box], p, q, tm[t], ob);
              if (k == 0x80000000u) ++deg;
              else if (k >> 31) return 2;
              sum += k;
              ++n;
            }
          }
  std::printf("%llu keys, %llu degenerate, sum %llu\n", n, deg, sum);
  return deg > 0 && deg < n ? 0 : 3;
}
"""


def test_key_header_is_clean_under_sanitizers(tmp_path):
    # a stand-alone program (its own main, no preloaded runtime) over the extreme inputs
    (tmp_path / "key_main.cpp").write_text(SANITIZED_MAIN)
    exe = tmp_path / "key_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover", "-I", str(ROOT / "my-raytracer_amd" / "csrc" / "device"),
                    "-o", str(exe), str(tmp_path / "key_main.cpp")], check=True, timeout=300)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "degenerate" in run.stdout


@pytest.mark.parametrize("ob", [0, -1])
def test_sorting_by_key_makes_a_shuffled_camera_coherent(ob):
    W, H = 256, 144
    rays = order_cases.pinhole_rays(W, H)
    shuffle = np.random.default_rng(3).permutation(W * H)
    shuffled = rays[shuffle]
    lo, hi = np.array([-4.0, -3.0, -9.0]), np.array([4.0, 3.0, 1.0])   # the eye inside the box
    keys = rtamd.ray_keys_host(lo, hi, shuffled, ob)
    order = np.argsort(keys, kind="stable")
    base = order_cases.mean_wave_bbox(shuffle, W)
    got = order_cases.mean_wave_bbox(shuffle[order], W)
    print(f"origin_bits {ob}: mean 64-ray pixel box {got:.0f} px sorted, {base:.0f} px shuffled, ratio {got / base:.4f}")
    assert got <= 0.05 * base
