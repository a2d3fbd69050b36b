"""rt_trace_hits C ABI without a GPU: the symbol, the constants, the layout of
rt_hit_key against a compiled C program, the argument checks made before any HIP call, and the
Python layer's own checks."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rtamd
from rtamd import abi

ROOT = Path(__file__).resolve().parents[1]


def test_hits_symbol_exported_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", str(rtamd.HIP_LIB)], capture_output=True, text=True,
                         check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    header = (ROOT / "include" / "rt_hip.h").read_text()
    assert "rt_trace_hits" in names
    assert "rt_trace_hits" in abi.HIP_SYMBOLS
    assert " rt_trace_hits(" in header
    assert len(rtamd.hip_lib().rt_trace_hits.argtypes) == 9
    assert "#define RT_HITS_MAX_K 8" in header
    assert "#define RT_HITS_MAX_ROWS (1LL << 31)" in header
    assert (abi.RT_HITS_MAX_K, abi.RT_HITS_MAX_ROWS) == (8, 1 << 31)


def test_hit_key_layout_matches_c(tmp_path):
    fields = ["t", "slot", "reserved_"]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rt_hip.h"', "int main(void){",
           'printf("%zu\\n", sizeof(rt_hit_key));']
    src += [f'printf("%zu\\n", offsetof(rt_hit_key, {f}));' for f in fields]
    src.append("return 0;}")
    (tmp_path / "key_sizes.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-o", str(tmp_path / "key_sizes"), str(tmp_path / "key_sizes.c")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "key_sizes")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [16, 0, 8, 12]
    assert got[0] == C.sizeof(abi.HitKey) == rtamd.HIT_KEY_DTYPE.itemsize
    assert got[1:] == [getattr(abi.HitKey, f).offset for f in fields]
    assert got[1:] == [rtamd.HIT_KEY_DTYPE.fields[f][1] for f in fields]


def _clear_error(lib):
    """Leaves another call's message in rt_last_error, so that a stale one cannot pass for a new one."""
    assert lib.rt_tile_shape(None, None) == abi.RT_ERR_INVALID
    assert lib.rt_last_error().startswith(b"rt_tile_shape:")


def test_trace_hits_rejects_bad_arguments_and_accepts_no_rays():
    # checked before any HIP call: no GPU needed.  The non-null scene pointer is never dereferenced.
    lib = rtamd.hip_lib()
    buf = (C.c_char * 1024)()
    p = C.c_void_p(C.addressof(buf))
    fake = C.cast((C.c_char * 16)(), C.c_void_p)
    rows = abi.RT_HITS_MAX_ROWS
    #        scene rays n  k  after hits count stats stream
    cases = [((None, p, 1, 1, None, p, p, None, None), b"null scene"),
             ((None, p, 0, 1, None, p, p, None, None), b"null scene"),
             ((fake, p, -1, 1, None, p, p, None, None), b"negative ray count"),
             ((fake, p, 1, 0, None, p, p, None, None), b"k outside"),
             ((fake, p, 1, -1, None, p, p, None, None), b"k outside"),
             ((fake, p, 1, abi.RT_HITS_MAX_K + 1, None, p, p, None, None), b"k outside"),
             ((fake, p, 0, 0, None, p, p, None, None), b"k outside"),
             ((fake, p, rows + 1, 1, None, p, p, None, None), b"RT_HITS_MAX_ROWS"),
             ((fake, p, rows // 8 + 1, 8, None, p, p, None, None), b"RT_HITS_MAX_ROWS"),
             ((fake, p, rows // 3 + 1, 3, None, p, p, None, None), b"RT_HITS_MAX_ROWS"),
             ((fake, None, 1, 1, None, p, p, None, None), b"null ray, result or count"),
             ((fake, p, 1, 1, None, None, p, None, None), b"null ray, result or count"),
             ((fake, p, 1, 1, p, p, None, None, None), b"null ray, result or count")]
    for args, why in cases:
        _clear_error(lib)
        assert lib.rt_trace_hits(*args) == abi.RT_ERR_INVALID, why
        msg = lib.rt_last_error()
        assert msg.startswith(b"rt_trace_hits:") and why in msg, (why, msg)
    # n = 0: nothing to do, whatever the buffers; the statistics are zeroed
    st = abi.QueryStats(rays=-1, hits=-1)
    assert lib.rt_trace_hits(fake, None, 0, 1, None, None, None, C.byref(st), None) == abi.RT_OK
    assert (st.rays, st.hits) == (0, 0)
    assert lib.rt_trace_hits(fake, None, 0, abi.RT_HITS_MAX_K, None, None, None, None, None) == abi.RT_OK


def test_python_layer_reports_a_library_without_the_symbol(monkeypatch):
    class Partial:   # what abi.bind(..., partial=True) leaves of a library built from an older source
        def __getattr__(self, name):
            raise AttributeError(name)

    with monkeypatch.context() as m:
        m.setattr(rtamd, "hip_lib", lambda: Partial())
        with pytest.raises(rtamd.RtError) as e:
            rtamd._hits_fn("rt_trace_hits")
    assert type(e.value) is rtamd.RtError and "rt_trace_hits" in str(e.value)


def test_hit_keys_of_the_python_layer():
    import torch

    cpu = torch.device("cpu")
    t, slot = np.array([0.5, -np.inf, np.nan]), np.array([7, -1, 2 ** 31 - 1])
    rec = np.zeros(3, rtamd.HIT_KEY_DTYPE)
    rec["t"], rec["slot"] = t, slot
    want = rec.view(np.int64).reshape(3, 2)
    for after in ((t, slot), rec, rec.view(np.float64).reshape(3, 2), (torch.from_numpy(t), torch.from_numpy(slot)),
                  torch.from_numpy(want.copy()), torch.from_numpy(rec.view(np.float64).reshape(3, 2).copy())):
        got = rtamd._hit_keys(after, 3, cpu)
        assert got.dtype == torch.int64 and got.is_contiguous() and np.array_equal(got.numpy(), want)
    for bad in ((t, slot, slot), rec[:2], np.zeros((3, 3)), (t[:2], slot[:2]), torch.zeros((3, 2), dtype=torch.float32)):
        with pytest.raises(ValueError):
            rtamd._hit_keys(bad, 3, cpu)
