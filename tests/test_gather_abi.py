"""rt_trace_gather without a GPU: symbol, declaration, binding, the argument checks
of rt_trace_radiance (render parameters) and rt_trace_ao (points, fan, buffers) before any HIP call,
n = 0, and DeviceScene.gather's own input checks."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rtamd
from rtamd import abi

import radiance_cases as rc

ROOT = Path(__file__).resolve().parents[1]


def test_gather_symbol_exported_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", str(rtamd.HIP_LIB)], capture_output=True, text=True,
                         check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert "rt_trace_gather" in names
    assert "rt_trace_gather" in abi.HIP_SYMBOLS
    header = (ROOT / "include" / "rt_hip.h").read_text()
    assert "int rt_trace_gather(" in header
    # the header says what the mean is and what is not built
    assert "CLAMPED PER SAMPLE" in header and "(HDR) sum and per-direction" in header
    fn = rtamd.hip_lib().rt_trace_gather
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert b"rt_trace_gather" in rtamd.hip_lib().rt_build_info()


def _good_params():
    hs, _ = rc.scene("cornell")
    return rc.params(hs, 8, 8)


def _fan(k=4, n_sets=2, seed=0, bias=0.0, dirs=True):
    buf = (C.c_double * 64)()
    a = abi.AoParams(k=k, n_sets=n_sets, seed=seed, bias=bias, d_dirs=C.addressof(buf) if dirs else None)
    a._keep = buf
    return a


def _clear_error(lib):
    """Leaves another call's message in rt_last_error, so that a stale one cannot pass for a new one."""
    assert lib.rt_tile_shape(None, None) == abi.RT_ERR_INVALID
    assert lib.rt_last_error().startswith(b"rt_tile_shape:")


def _rejected(lib, args, why=b""):
    _clear_error(lib)
    assert lib.rt_trace_gather(*args) == abi.RT_ERR_INVALID, (args, why)
    msg = lib.rt_last_error()
    assert msg and not msg.startswith(b"rt_tile_shape:") and why in msg, (why, msg)


def test_gather_rejects_what_radiance_rejects_about_the_render_parameters():
    # no GPU here: a non-null scene pointer is never dereferenced before the checks
    lib = rtamd.hip_lib()
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    p = _good_params()
    ok = _fan()
    _rejected(lib, (None, C.byref(p), ptr, 1, C.byref(ok), ptr, None, None), b"null scene")
    _rejected(lib, (None, C.byref(p), ptr, 0, C.byref(ok), ptr, None, None), b"null scene")
    _rejected(lib, (fake, None, ptr, 1, C.byref(ok), ptr, None, None), b"null scene or params")
    flags = [abi.RT_FLAG_TRAVERSAL_STATS, abi.RT_FLAG_WIDE_STATS, abi.RT_FLAG_TIMELINE, abi.RT_FLAG_TILE_COST,
             abi.RT_FLAG_TILE_COST_TIME, abi.RT_FLAG_COST_ORDER, abi.RT_FLAG_GLOBAL_ROWS,
             abi.RT_FLAG_NATURAL_ORDER | abi.RT_FLAG_COST_ORDER, 1 << 20]
    bad_fields = [({"spp_n": 2}, b"spp_n"), ({"spp_n": 0}, b"spp_n"), ({"row_begin": 1}, b"row ranges"),
                  ({"row_end": 4}, b"row ranges"), ({"stripe_count": 2}, b"stripes"),
                  ({"stripe_count": 2, "stripe_index": 1}, b"stripes"), ({"stripe_index": 1}, b"stripes"),
                  ({"out_format": 2}, b"out_format"), ({"out_format": -1}, b"out_format"),
                  ({"max_depth": -1}, b"max_depth"), ({"n_lights": -1}, b"n_lights")]
    bad_fields += [({"flags": f}, b"RT_FLAG_NATURAL_ORDER") for f in flags]
    for fields, why in bad_fields:
        q = rc.copy_params(p, **fields)
        for n in (1, 0):   # checked whatever the count
            _rejected(lib, (fake, C.byref(q), ptr, n, C.byref(ok), ptr, None, None), why)


BAD_FANS = [(dict(k=0), b"k outside"), (dict(k=-3), b"k outside"), (dict(k=1025), b"k outside"),
            (dict(n_sets=0), b"n_sets outside"), (dict(n_sets=65537), b"n_sets outside"),
            (dict(bias=float("nan")), b"bias"), (dict(bias=float("inf")), b"bias"),
            (dict(bias=float("-inf")), b"bias"), (dict(dirs=False), b"null point, direction or result")]


def test_gather_rejects_what_ao_rejects_about_points_fan_and_buffers():
    lib = rtamd.hip_lib()
    buf = (C.c_char * 1024)()
    ptr = C.c_void_p(C.addressof(buf))
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    p = _good_params()
    P = C.byref(p)
    ok = _fan()
    cases = [((fake, P, ptr, 1, None, ptr, None, None), b"null parameters"),
             ((fake, P, ptr, -1, C.byref(ok), ptr, None, None), b"negative point count"),
             ((fake, P, ptr, (1 << 31) + 1, C.byref(ok), ptr, None, None), b"RT_AO_MAX_POINTS"),
             ((fake, P, None, 1, C.byref(ok), ptr, None, None), b"null point, direction or result"),
             ((fake, P, ptr, 1, C.byref(ok), None, None, None), b"null point, direction or result")]
    keep = []
    for kw, why in BAD_FANS:
        keep.append(_fan(**kw))
        cases.append(((fake, P, ptr, 1, C.byref(keep[-1]), ptr, None, None), why))
    for args, why in cases:
        _rejected(lib, args, why)
        assert lib.rt_last_error().startswith(b"rt_trace_gather:")


def test_gather_of_no_points_is_ok_without_a_device():
    # n == 0 with valid arguments returns before any HIP call, buffers may be null, stats are zeroed
    lib = rtamd.hip_lib()
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    p = _good_params()
    for flags in (0, abi.RT_FLAG_NATURAL_ORDER):
        q = rc.copy_params(p, flags=flags)
        st = abi.Stats(primary_rays=-1, pixels=-1)
        fan = _fan(dirs=False)
        assert lib.rt_trace_gather(fake, C.byref(q), None, 0, C.byref(fan), None, C.byref(st), None) == abi.RT_OK
        assert (st.primary_rays, st.shadow_rays, st.reflection_rays, st.pixels) == (0, 0, 0, 0)
    # the limits themselves pass the checks
    for fan in (_fan(k=abi.RT_AO_MAX_SAMPLES), _fan(n_sets=abi.RT_AO_MAX_SETS)):
        assert lib.rt_trace_gather(fake, C.byref(p), None, 0, C.byref(fan), None, None, None) == abi.RT_OK


def _bare_scene():
    dev = object.__new__(rtamd.DeviceScene)   # no upload: the checks come first
    dev.device = 0
    dev._h = None
    return dev


def test_gather_method_checks_its_inputs_before_calling_the_library():
    import torch

    dev = _bare_scene()
    p = _good_params()
    good_pts, good_dirs = np.zeros((4, 8)), np.zeros((1, 2, 3))
    for pts in (np.zeros((4, 7)), np.zeros(8), np.zeros((2, 4, 8)),              # shape
                torch.zeros((4, 8), dtype=torch.float32),                        # dtype
                torch.zeros((4, 8), dtype=torch.float64),                        # device (a CPU tensor)
                torch.zeros((4, 7), dtype=torch.float64),
                torch.zeros((8, 8), dtype=torch.float64)[::2],                   # not contiguous
                [[0.0] * 8]):
        with pytest.raises(ValueError, match="points"):
            dev.gather(pts, good_dirs, p)
    for dirs in (np.zeros((1, 3)), np.zeros((1, 2, 4)), np.zeros((1, 1, 2, 3)),
                 torch.zeros((1, 2, 3), dtype=torch.float32),
                 torch.zeros((1, 2, 3), dtype=torch.float64),                    # not on the device
                 torch.zeros((1, 4, 3), dtype=torch.float64)[:, ::2],
                 [[[0.0, 0.0, 1.0]]]):
        with pytest.raises(ValueError, match="dirs"):
            dev.gather(good_pts, dirs, p)


def test_gather_method_reports_a_library_without_the_symbol(monkeypatch):
    class Partial:   # what abi.bind(..., partial=True) leaves of a library built from an older source
        def __getattr__(self, name):
            raise AttributeError(name)

    p = _good_params()
    dev = _bare_scene()
    monkeypatch.setattr(rtamd, "hip_lib", lambda: Partial())
    with pytest.raises(rtamd.RtError) as e:
        dev.gather(np.zeros((1, 8)), np.zeros((1, 1, 3)), p)
    assert type(e.value) is rtamd.RtError and "rt_trace_gather" in str(e.value)
