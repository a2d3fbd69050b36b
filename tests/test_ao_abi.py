"""Occlusion-fan C ABI without a GPU: symbols, argument checks, rt_ao_rays_host
against its numpy restatement (ao_cases.numpy_rays) bit for bit, the fan header under UBSan / ASan in
a stand-alone program on the same inputs, and the direction sets of ao_directions."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rtamd
from rtamd import abi

import ao_cases

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = {"rt_trace_ao": 7, "rt_ao_rays_host": 4}


def test_ao_symbols_exported_declared_and_bound():
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
    for macro, value in (("RT_AO_MAX_SAMPLES", "1024"), ("RT_AO_MAX_SETS", "65536"), ("RT_AO_MAX_POINTS", "(1LL << 31)")):
        assert f"#define {macro} {value}" in header
    assert (abi.RT_AO_MAX_SAMPLES, abi.RT_AO_MAX_SETS, abi.RT_AO_MAX_POINTS) == (1024, 65536, 1 << 31)
    assert (ao_cases.K_MAX, ao_cases.SETS_MAX) == (abi.RT_AO_MAX_SAMPLES, abi.RT_AO_MAX_SETS)


def test_ao_params_layout_matches_c(tmp_path):
    fields = ["k", "n_sets", "seed", "reserved_", "bias", "d_dirs"]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rt_hip.h"', "int main(void){",
           'printf("%zu\\n", sizeof(rt_ao_params));']
    src += [f'printf("%zu\\n", offsetof(rt_ao_params, {f}));' for f in fields]
    src.append("return 0;}")
    (tmp_path / "ao_sizes.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-o", str(tmp_path / "ao_sizes"), str(tmp_path / "ao_sizes.c")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "ao_sizes")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got[0] == C.sizeof(abi.AoParams)
    assert got[1:] == [getattr(abi.AoParams, f).offset for f in fields]


def _clear_error(lib):
    """Leaves another call's message in rt_last_error, so that a stale one cannot pass for a new one."""
    assert lib.rt_tile_shape(None, None) == abi.RT_ERR_INVALID
    assert lib.rt_last_error().startswith(b"rt_tile_shape:")


def _params(k=4, n_sets=2, seed=0, bias=0.0, dirs=True):
    buf = (C.c_double * 64)()
    a = abi.AoParams(k=k, n_sets=n_sets, seed=seed, bias=bias, d_dirs=C.addressof(buf) if dirs else None)
    a._keep = buf
    return a


BAD_PARAMS = [(dict(k=0), b"k outside"), (dict(k=-3), b"k outside"), (dict(k=1025), b"k outside"),
              (dict(n_sets=0), b"n_sets outside"), (dict(n_sets=65537), b"n_sets outside"),
              (dict(bias=float("nan")), b"bias"), (dict(bias=float("inf")), b"bias"),
              (dict(bias=float("-inf")), b"bias"), (dict(dirs=False), b"null point, direction or result")]


def test_trace_ao_rejects_bad_arguments():
    # checked before any HIP call: no GPU needed.  The non-null scene pointer is never dereferenced.
    lib = rtamd.hip_lib()
    buf = (C.c_char * 1024)()
    p = C.c_void_p(C.addressof(buf))
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    ok = _params()
    cases = [((None, p, 1, C.byref(ok), p, None, None), b"null scene"),
             ((None, p, 0, C.byref(ok), p, None, None), b"null scene"),
             ((fake, p, 1, None, p, None, None), b"null parameters"),
             ((fake, p, -1, C.byref(ok), p, None, None), b"negative point count"),
             ((fake, p, (1 << 31) + 1, C.byref(ok), p, None, None), b"RT_AO_MAX_POINTS"),
             ((fake, None, 1, C.byref(ok), p, None, None), b"null point, direction or result"),
             ((fake, p, 1, C.byref(ok), None, None, None), b"null point, direction or result")]
    keep = []
    for kw, why in BAD_PARAMS:
        keep.append(_params(**kw))
        cases.append(((fake, p, 1, C.byref(keep[-1]), p, None, None), why))
    for args, why in cases:
        _clear_error(lib)
        assert lib.rt_trace_ao(*args) == abi.RT_ERR_INVALID, why
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_trace_ao:") and why in msg, (why, msg)


def test_ao_rays_host_rejects_bad_arguments_and_accepts_no_points():
    lib = rtamd.hip_lib()
    buf = (C.c_char * 1024)()
    p = C.c_void_p(C.addressof(buf))
    ok = _params()
    cases = [((p, 1, None, p), b"null parameters"), ((p, -1, C.byref(ok), p), b"negative point count"),
             ((p, (1 << 31) + 1, C.byref(ok), p), b"RT_AO_MAX_POINTS"),
             ((None, 1, C.byref(ok), p), b"null point, direction or result"),
             ((p, 1, C.byref(ok), None), b"null point, direction or result")]
    keep = []
    for kw, why in BAD_PARAMS:
        keep.append(_params(**kw))
        cases.append(((p, 1, C.byref(keep[-1]), p), why))
    for args, why in cases:
        _clear_error(lib)
        assert lib.rt_ao_rays_host(*args) == abi.RT_ERR_INVALID, why
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_ao_rays_host:") and why in msg, (why, msg)
    # n = 0: nothing to do, whatever the pointers
    assert lib.rt_ao_rays_host(None, 0, C.byref(_params(dirs=False)), None) == abi.RT_OK
    assert rtamd.ao_rays_host(np.zeros((0, 8)), np.zeros((2, 4, 3))).shape == (0, 8)
    # the limits themselves are accepted
    one = np.zeros((1, 8))
    assert rtamd.ao_rays_host(one, np.zeros((1, abi.RT_AO_MAX_SAMPLES, 3))).shape == (abi.RT_AO_MAX_SAMPLES, 8)
    assert rtamd.ao_rays_host(one, np.zeros((abi.RT_AO_MAX_SETS, 1, 3))).shape == (1, 8)


def test_python_layer_reports_a_library_without_the_symbols(monkeypatch):
    class Partial:   # what abi.bind(..., partial=True) leaves of a library built from an older source
        def __getattr__(self, name):
            raise AttributeError(name)

    dev = object.__new__(rtamd.DeviceScene)
    dev.device = 0
    dev._h = None
    monkeypatch.setattr(rtamd, "hip_lib", lambda: Partial())
    for call, sym in ((lambda: dev.ao(np.zeros((1, 8)), np.zeros((1, 1, 3))), "rt_trace_ao"),
                      (lambda: rtamd.ao_rays_host(np.zeros((1, 8)), np.zeros((1, 1, 3))), "rt_ao_rays_host")):
        with pytest.raises(rtamd.RtError) as e:
            call()
        assert type(e.value) is rtamd.RtError and sym in str(e.value)


def test_python_layer_checks_its_inputs():
    with pytest.raises(ValueError):
        rtamd.ao_rays_host(np.zeros((4, 7)), np.zeros((1, 1, 3)))
    with pytest.raises(ValueError):
        rtamd.ao_rays_host(np.zeros((4, 8)), np.zeros((1, 3)))
    with pytest.raises(ValueError):
        rtamd.ao_directions(0, 1)
    with pytest.raises(ValueError):
        rtamd.ao_directions(4, abi.RT_AO_MAX_SETS + 1)


@pytest.fixture(scope="module")
def host_points():
    return ao_cases.host_points()


@pytest.mark.parametrize("n_sets", [1, 7])
@pytest.mark.parametrize("bias", [0.0, 1e-3])
def test_host_rays_equal_the_numpy_fan(host_points, n_sets, bias):
    well, pts = host_points
    dirs = ao_cases.host_dirs(n_sets)
    k = dirs.shape[1]
    seed = 0x9e3779b9
    got = rtamd.ao_rays_host(pts, dirs, seed, bias)
    want = ao_cases.numpy_rays(pts, dirs, seed, bias)
    assert got.shape == (len(pts) * k, 8) and ao_cases.same_bits(got, want)
    # degenerate points: Ray(o, 0) with their own tmax
    bad = ~ao_cases.numpy_valid(pts)
    nd = len(ao_cases.degenerate_points())
    assert bad.sum() == nd
    g = got.reshape(len(pts), k, 8)
    assert np.all(g[bad][:, :, 3:6] == 0.0)
    assert ao_cases.same_bits(g[bad][:, :, 0:3], np.repeat(pts[bad][:, None, 0:3], k, 1))
    assert ao_cases.same_bits(g[:, :, 6], np.repeat(pts[:, 6:7], k, 1)) and np.all(g[:, :, 7] == 0.0)
    # sample 0 is the zero direction (a degenerate ray), sample 3 has a NaN: nothing is clamped
    ok = ~bad
    assert np.all(g[ok][:, 0, 3:6] == 0.0) and np.all(np.isnan(g[ok][:, 3, 3:6]).any(axis=1))
    # sample 1 is the normal itself: w = N, and the origin moves along it by the bias
    N, T, B = ao_cases.numpy_frame(well[:, 3:6])
    nw = len(well)
    assert ao_cases.same_bits(g[:nw, 1, 3:6], (0.0 * T + 0.0 * B) + 1.0 * N)
    assert ao_cases.same_bits(g[:nw, 1, 0:3], well[:, 0:3] + bias * N)


def test_frame_is_orthonormal(host_points):
    well, _ = host_points
    N, T, B = ao_cases.numpy_frame(well[:, 3:6])
    assert np.any(N[:, 2] == -1.0) and np.any(N[:, 2] == 1.0)
    for u, v in ((T, B), (T, N), (B, N)):
        assert np.max(np.abs((u * v).sum(1))) <= 1e-14
    for u in (T, B, N):
        assert np.max(np.abs(np.sqrt((u * u).sum(1)) - 1.0)) <= 1e-14
    # right-handed: T x B = N
    assert np.max(np.abs(np.cross(T, B) - N)) <= 1e-14
    # ... and the library's rays carry that frame: local x, y, z come out as T, B, N
    dirs = np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]])
    g = rtamd.ao_rays_host(well, dirs).reshape(len(well), 3, 8)
    for s, u in enumerate((T, B, N)):
        assert np.array_equal(g[:, s, 3:6] + 0.0, u + 0.0)   # (+ 0.0: -0.0 == 0.0 either way)


@pytest.mark.parametrize("seed,n_sets", [(0, 7), (12345, 7), (0xffffffff, 1000), (7, 1), (3, 65536)])
def test_set_index_equals_the_numpy_hash(seed, n_sets):
    # normal +z: T = x, B = y, N = z, so the fan ray is the local direction itself; the table
    # stores (set, sample, 1)
    n, k = 3000, 2
    pts = ao_cases.make_points(np.zeros((n, 3)), np.tile([0.0, 0.0, 1.0], (n, 1)))
    dirs = np.zeros((n_sets, k, 3))
    dirs[:, :, 0] = np.arange(n_sets)[:, None]
    dirs[:, :, 1] = np.arange(k)[None, :]
    dirs[:, :, 2] = 1.0
    g = rtamd.ao_rays_host(pts, dirs, seed).reshape(n, k, 8)
    sets = ao_cases.numpy_sets(n, seed, n_sets)
    assert np.array_equal(g[:, :, 3], np.repeat(sets[:, None].astype(np.float64), k, 1))
    assert np.array_equal(g[:, :, 4], np.tile(np.arange(k, dtype=np.float64), (n, 1)))
    if n_sets >= 7:
        assert len(np.unique(sets)) >= 7
    # the mixer's fixed points of reference: 0 -> 0, and a bijection on a sample
    assert int(ao_cases.numpy_hash([0])[0]) == 0
    assert len(np.unique(ao_cases.numpy_hash(np.arange(1 << 16)))) == 1 << 16


SANITIZED_MAIN = r"""
#include "rt_ao_fan.hpp"
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
int main(int argc, char** argv) {
  if (argc != 8) return 5;
  const std::vector<double> pts = slurp(argv[1]), dirs = slurp(argv[2]);
  const int k = std::atoi(argv[3]), n_sets = std::atoi(argv[4]);
  const uint32_t seed = (uint32_t)std::strtoul(argv[5], nullptr, 10);
  const double bias = std::atof(argv[6]);
  const long long n = (long long)(pts.size() / 8);
  if (dirs.size() != (size_t)n_sets * k * 3) return 6;
  std::vector<double> rays((size_t)n * k * 8, 0.0);
  unsigned long long degenerate = 0;
  for (long long i = 0; i < n; ++i) {
    const double* pt = &pts[(size_t)i * 8];
    if (!rt_ao_point_valid(pt, pt + 3, pt[6])) ++degenerate;
    const size_t set = rt_ao_set(i, seed, n_sets);
    for (int s = 0; s < k; ++s) {
      double* r = &rays[((size_t)i * k + s) * 8];
      rt_ao_fan_ray(pt, pt + 3, pt[6], &dirs[(set * k + s) * 3], bias, r, r + 3);
      r[6] = pt[6];
    }
  }
  FILE* f = std::fopen(argv[7], "wb");
  if (!f || std::fwrite(rays.data(), sizeof(double), rays.size(), f) != rays.size()) return 7;
  std::fclose(f);
  std::printf("%lld points, %llu degenerate, hash(1) = %u\n", n, degenerate, rt_ao_hash(1u));
  return 0;
}
"""


def test_fan_header_is_clean_under_sanitizers(tmp_path, host_points):
    # a stand-alone program (its own main, no preloaded runtime) over the inputs of the numpy test
    _, pts = host_points
    dirs = ao_cases.host_dirs(7)
    k, seed, bias = dirs.shape[1], 0x9e3779b9, 1e-3
    (tmp_path / "fan_main.cpp").write_text(SANITIZED_MAIN)
    pts.tofile(tmp_path / "pts.bin")
    dirs.tofile(tmp_path / "dirs.bin")
    exe = tmp_path / "fan_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover", "-I", str(ROOT / "my-raytracer_amd" / "csrc" / "device"),
                    "-o", str(exe), str(tmp_path / "fan_main.cpp")], check=True, timeout=300)
    run = subprocess.run([str(exe), str(tmp_path / "pts.bin"), str(tmp_path / "dirs.bin"), str(k), "7", str(seed),
                          repr(bias), str(tmp_path / "rays.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{len(ao_cases.degenerate_points())} degenerate" in run.stdout
    assert f"hash(1) = {int(ao_cases.numpy_hash([1])[0])}" in run.stdout
    got = np.fromfile(tmp_path / "rays.bin").reshape(-1, 8)
    assert ao_cases.same_bits(got, rtamd.ao_rays_host(pts, dirs, seed, bias))


@pytest.mark.parametrize("k,n_sets", [(64, 1024), (16, 4096), (1, 65536), (100, 7)])
@pytest.mark.parametrize("cosine", [True, False])
def test_ao_directions(k, n_sets, cosine):
    d = rtamd.ao_directions(k, n_sets, seed=5, cosine=cosine)
    assert d.shape == (n_sets, k, 3) and d.dtype == np.float64 and d.flags["C_CONTIGUOUS"]
    assert np.all(d[..., 2] > 0.0)
    assert np.max(np.abs(np.sqrt((d * d).sum(2)) - 1.0)) <= 1e-15
    assert np.array_equal(d, rtamd.ao_directions(k, n_sets, seed=5, cosine=cosine))   # a function of the seed
    assert not np.array_equal(d, rtamd.ao_directions(k, n_sets, seed=6, cosine=cosine))
    if k * n_sets == 65536:
        # 5 standard errors of the mean of 65 536 independent samples (stratified ones vary less):
        # cosine: var z = 1/2 - 4/9 = 1/18, sqrt(1/18) / 256 = 0.00092; uniform: var z = 1/12
        mean = d[..., 2].mean()
        print(f"k {k} sets {n_sets} cosine {cosine}: mean z {mean:.5f}")
        assert abs(mean - (2.0 / 3.0 if cosine else 0.5)) <= (0.005 if cosine else 0.006)
        assert abs(d[..., 0].mean()) <= 0.01 and abs(d[..., 1].mean()) <= 0.01   # the sets' own rotations
    if k >= 16:
        # stratified: in every set each of the k equal-probability bands of z holds one sample
        u = 1.0 - d[..., 2] ** 2 if cosine else 1.0 - d[..., 2]
        band = np.clip(np.floor(u * k + 1e-9 * k).astype(np.int64), 0, k - 1)
        assert np.mean(np.sort(band, axis=1) == np.arange(k)[None, :]) >= 0.99
