"""Rays and oracle expectations shared by tests/test_query_abi.py and tests/test_query_gpu.py.

Every expected value comes from the CPU oracle (pyoracle.Oracle.closest_hit,
pyoracle.intersect_triangle).  Expectations are computed once per (scene, ray set, mode) and shared;
callers must not modify them."""
import functools
import math

import numpy as np

import pyoracle
import rtamd

SCENES = {"cornell": {}, "office": {}, "random_tris": {"n_triangles": 20000}}


@functools.lru_cache(maxsize=None)
def scene(name, n_triangles=0):
    """(HostScene, Oracle, vertex positions, vertex_idx, perm) of a generated scene."""
    hs = rtamd.HostScene.generate(name, n_triangles=n_triangles)
    hs.prepare()
    orc = pyoracle.Oracle(hs.raw, hs)
    soa = hs.soa_arrays()
    return hs, orc, soa["vertex_pos"], soa["vertex_idx"], orc.bvh()["perm"]


def root_box(hs):
    b = hs.bvh_arrays()
    return b["bb_min"][0].copy(), b["bb_max"][0].copy()


def make_rays(o, d, tmax=np.inf):
    rays = np.zeros((len(o), 8))
    rays[:, 0:3] = o
    rays[:, 3:6] = d
    rays[:, 6] = tmax
    return rays


def origins(hs, u):
    lo, hi = root_box(hs)
    ext = hi - lo
    return lo - 0.25 * ext + u * 1.5 * ext


def random_rays(hs, n=4096, seed=7):
    """Case 1: origins around the root box, normal-distributed directions (o drawn first)."""
    rng = np.random.default_rng(seed)
    o = origins(hs, rng.random((n, 3)))
    d = rng.normal(size=(n, 3))
    return make_rays(o, d)


def vertex_rays(hs, P, n=2048, seed=5):
    """Case 3: every ray aimed at a mesh vertex (ties and edges)."""
    rng = np.random.default_rng(seed)
    o = origins(hs, rng.random((n, 3)))
    d = P[rng.integers(0, len(P), n)] - o
    return make_rays(o, d)


def axis_rays(hs, n=2048, seed=5):
    """Case 4: axis-aligned directions (two zero components: clamped reciprocals)."""
    rng = np.random.default_rng(seed)
    o = origins(hs, rng.random((n, 3)))
    axis = rng.integers(0, 3, n)
    sign = rng.choice([-1.0, 1.0], n)
    d = np.zeros((n, 3))
    d[np.arange(n), axis] = sign
    return make_rays(o, d)


def oracle_hits(orc, rays, mode):
    """The oracle's closest hit of every ray: dict of hit [n] bool, t, tri, normal [n, 3], point [n, 3]."""
    n = len(rays)
    out = {"hit": np.zeros(n, bool), "t": np.full(n, np.inf), "tri": np.full(n, -1, np.int64),
           "normal": np.zeros((n, 3)), "point": np.zeros((n, 3))}
    for i in range(n):
        h = orc.closest_hit(rays[i, 0:3], rays[i, 3:6], mode)
        if h is not None:
            out["hit"][i] = True
            out["t"][i] = h["t"]
            out["tri"][i] = h["tri"]
            out["normal"][i] = h["normal"]
            out["point"][i] = h["point"]
    return out


_expect = {}


def expected(key, orc, rays, mode):
    """oracle_hits, computed once per key."""
    k = (key, mode)
    if k not in _expect:
        _expect[k] = oracle_hits(orc, rays, mode)
    return _expect[k]


def normalized(d):
    x, y, z = float(d[0]), float(d[1]), float(d[2])
    n = math.sqrt(x * x + y * y + z * z)
    return np.array([x / n, y / n, z / n])


def check_hits(got, want, rays, P, vidx, perm, analytic=False, only=None):
    """Exact comparison of a closest-hit result (dict of numpy arrays) with the oracle's.
    only: optional boolean mask of the rays to compare."""
    idx = np.arange(len(rays)) if only is None else np.nonzero(only)[0]
    hit = np.isfinite(got["t"])
    assert np.array_equal(hit[idx], want["hit"][idx])
    assert np.array_equal(got["t"][idx], want["t"][idx])
    assert np.array_equal(got["normal"][idx], want["normal"][idx])
    for i in idx:
        slot, prim, mesh = int(got["slot"][i]), int(got["prim"][i]), int(got["mesh"][i])
        if not hit[i]:
            assert (slot, mesh, prim) == (-1, -1, -1)
            assert got["alpha"][i] == 0.0 and got["beta"][i] == 0.0
            continue
        if want["tri"][i] < 0:
            assert analytic and slot == -1 and mesh == -1 and prim >= 0
            assert got["alpha"][i] == 0.0 and got["beta"][i] == 0.0
            continue
        assert prim == -1 and mesh >= 0
        assert perm[slot] == want["tri"][i]
        v = vidx[slot]
        tab = pyoracle.intersect_triangle(P[v[0]], P[v[1]], P[v[2]], rays[i, 0:3], normalized(rays[i, 3:6]))
        assert tab is not None
        assert tab[0] == got["t"][i]
        assert tab[1] == got["alpha"][i] and tab[2] == got["beta"][i]
