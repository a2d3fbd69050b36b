"""Rays and oracle expectations shared by tests/test_radiance_abi.py and tests/test_radiance_gpu.py.

Every expected colour comes from the CPU oracle.  The oracle forms a primary direction as
lower_left + x * x_dir + y * y_dir - eye, so an arbitrary ray (o, target - o) is the one pixel of a
1 x 1 camera with eye = o, lower_left = target and x_dir = y_dir = 0: the same single subtraction
the test does in numpy.  Rays that share an origin go through one Oracle.render of a small camera
(rtamd.camera_rays gives that camera's rays).  Expectations are computed once and shared; callers
must not modify them."""
import numpy as np

import pyoracle
import rtamd
from rtamd import abi

import query_cases as qc

REF = pyoracle.MODE_REFERENCE
TOL64 = 1e-12   # fp64 output against the oracle, as tests/test_gpu_parity.py


def scene(name):
    """(HostScene, Oracle) of a generated scene of query_cases.SCENES."""
    hs, orc, _, _, _ = qc.scene(name, qc.SCENES[name].get("n_triangles", 0))
    return hs, orc


def counts(st):
    return [int(st.primary_rays), int(st.shadow_rays), int(st.reflection_rays)]


def params(hs, w, h, fmt=None):
    p = hs.render_params(w, h, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64 if fmt is None else fmt
    return p


def copy_params(p, **fields):
    q = abi.RenderParams.from_buffer_copy(p)
    for k, v in fields.items():
        setattr(q, k, v)
    return q


def with_eye(p, eye):
    """p with its camera moved rigidly so that its eye is `eye`."""
    q = copy_params(p)
    shift = np.asarray(eye, dtype=np.float64) - np.array(p.camera.eye[:])
    q.camera.eye[:] = [float(v) for v in np.array(p.camera.eye[:]) + shift]
    q.camera.lower_left[:] = [float(v) for v in np.array(p.camera.lower_left[:]) + shift]
    return q


_cache = {}


def oracle_frame(key, orc, p):
    """(image [H, W, 3], [primary, shadow, reflection]) of Oracle.render(p), once per key."""
    if key not in _cache:
        img, cnt = orc.render(p, REF)
        _cache[key] = (img, [int(cnt.primary_rays), int(cnt.shadow_rays), int(cnt.reflection_rays)])
    return _cache[key]


def oracle_single_rays(key, orc, p, o, target):
    """(colours [n, 3], summed [primary, shadow, reflection]) of the rays o[i] -> target[i], each
    the one pixel of a 1 x 1 oracle camera; once per key."""
    if key not in _cache:
        q = copy_params(p, spp_n=1, row_begin=0, row_end=0, stripe_height=1, stripe_count=1, stripe_index=0)
        q.camera.width = q.camera.height = 1
        q.camera.x_dir[:] = [0.0, 0.0, 0.0]
        q.camera.y_dir[:] = [0.0, 0.0, 0.0]
        rgb = np.zeros((len(o), 3))
        total = [0, 0, 0]
        for i in range(len(o)):
            q.camera.eye[:] = [float(v) for v in o[i]]
            q.camera.lower_left[:] = [float(v) for v in target[i]]
            img, cnt = orc.render(q, REF, threads=1)
            rgb[i] = img[0, 0]
            for k, v in enumerate((cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays)):
                total[k] += int(v)
        _cache[key] = (rgb, total)
    return _cache[key]


def arbitrary_rays(hs, n=256, seed=11):
    """(o, target, rays): origins drawn as query_cases.origins does, around and outside the root box;
    the first half of the targets inside the box (in the generated scenes nearly every such ray
    hits), the other half drawn like the origins, so that a good share of the rays miss;
    d = target - o, no component zero."""
    rng = np.random.default_rng(seed)
    lo, hi = qc.root_box(hs)
    o = qc.origins(hs, rng.random((n, 3)))
    target = lo + rng.random((n, 3)) * (hi - lo)
    target[n // 2:] = qc.origins(hs, rng.random((n - n // 2, 3)))
    d = target - o
    assert np.all(d != 0.0) and np.all(o != 0.0) and np.all(target != 0.0)
    return o, target, qc.make_rays(o, d)


def hit_distances(key, orc, rays):
    """(hit [n] bool, t [n]) of the oracle's closest hit of every ray; once per key."""
    if key not in _cache:
        want = qc.oracle_hits(orc, rays, REF)
        _cache[key] = (want["hit"], want["t"])
    return _cache[key]


def background(p):
    return np.minimum(np.array(p.background[:]), 1.0)


def degenerate_rows(good):
    """Copies of the valid rays `good`, each made degenerate in one way."""
    bad = []
    for col, val in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, -np.inf),
                     (6, np.nan), (6, 0.0), (6, 1e-5), (6, -1.0)):
        r = good.copy()
        r[:, col] = val
        bad.append(r)
    z = good.copy()
    z[:, 3:6] = 0.0
    bad.append(z)
    return np.concatenate(bad)
