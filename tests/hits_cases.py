"""Hit lists shared by tests/test_hits_gpu.py: the list H of rt_trace_hits (include/rt_hip.h) built
without the code under test.

Per ray a numpy fp64 restatement of the triangle test picks a candidate set with generous slack -- a
superset: widening the slack tenfold adds no confirmed hit, asserted for every list built -- and each
candidate is confirmed by the CPU's own test, pyoracle.intersect_triangle, on the slot's vertices and
the direction normalised by query_cases.normalized.  t, alpha and beta are that call's; the normal is
rt_trace_closest's documented rule applied to the uploaded normal arrays.  Lists are computed once
per key and shared; callers must not modify them."""
import numpy as np

import pyoracle
from rtamd import abi

import query_cases as qc

SLACK = 1e-6
HIT_DTYPE = np.dtype([("t", "<f8"), ("alpha", "<f8"), ("beta", "<f8"), ("normal", "<f8", (3,)), ("slot", "<i4"),
                      ("mesh", "<i4"), ("prim", "<i4"), ("reserved_", "<i4")])
assert HIT_DTYPE.itemsize == 64
MISS = np.zeros((), HIT_DTYPE)
MISS["t"], MISS["slot"], MISS["mesh"], MISS["prim"] = np.inf, -1, -1, -1


def _det3(a, b, c):
    return (a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1])
            - a[..., 1] * (b[..., 0] * c[..., 2] - b[..., 2] * c[..., 0])
            + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]))


class Geometry:
    """The uploaded arrays a hit list needs, per reference slot."""

    def __init__(self, hs):
        soa = hs.soa_arrays()
        s = hs.soa.contents
        self.P, self.vidx = soa["vertex_pos"], soa["vertex_idx"]
        self.vn, self.fn = soa["vertex_normals"], soa["face_normals"]
        self.mesh = soa["vertex_mesh_id"][self.vidx[:, 0]]
        self.draw = np.ctypeslib.as_array(s.mesh_draw_mode, (s.n_meshes,)).copy()
        self.p0, self.p1, self.p2 = (self.P[self.vidx[:, c]] for c in range(3))
        self.c1, self.c2 = self.p0 - self.p2, self.p1 - self.p2


def candidates(g, o, d, slack):
    """Slots whose triangle the ray (o, normalised d) may hit: the fp64 test with every bound loosened."""
    with np.errstate(all="ignore"):
        c3, c4 = -d[None, :], o[None, :] - g.p2
        S = _det3(g.c1, g.c2, c3)
        a = _det3(c4, g.c2, c3) / S
        b = _det3(g.c1, c4, c3) / S
        t = _det3(g.c1, g.c2, c4) / S
        ok = (np.abs(S) >= 1e-10 * (1.0 - slack)) & (a >= -slack) & (b >= -slack) & (a + b <= 1.0 + slack) & \
             (t > 1e-5 * (1.0 - slack))
    return np.nonzero(ok)[0]


def hit_list(g, ray):
    """H of one ray: a HIT_DTYPE array sorted by (t, slot).  A degenerate ray's list is empty."""
    o, dv, tmax = ray[0:3], ray[3:6], ray[6]
    with np.errstate(all="ignore"):
        dlen = np.sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2])
    if not (np.all(np.isfinite(o)) and np.all(np.isfinite(dv)) and dlen > 0.0 and tmax > 1e-5):
        return np.zeros(0, HIT_DTYPE)
    d = qc.normalized(dv)

    def confirmed(slots):
        out = []
        for s in slots:
            tab = pyoracle.intersect_triangle(g.p0[s], g.p1[s], g.p2[s], o, d)
            if tab is not None and 1e-5 < tab[0] < tmax and tab[0] != np.finfo(np.float64).max:
                out.append((tab[0], int(s), tab[1], tab[2]))
        return sorted(out)

    near = candidates(g, o, d, SLACK)
    hits = confirmed(near)
    wide = np.setdiff1d(candidates(g, o, d, 10.0 * SLACK), near)
    assert not confirmed(wide), "the candidate set is no superset of the hit list"
    H = np.zeros(len(hits), HIT_DTYPE)
    for j, (t, s, a, b) in enumerate(hits):
        gamma = 1.0 - a - b
        m = int(g.mesh[s])
        if g.draw[m] == abi.RT_DRAW_FLAT:
            n = g.fn[s]
        else:
            v = g.vidx[s]
            n = a * g.vn[v[0]] + b * g.vn[v[1]] + gamma * g.vn[v[2]]
        H[j] = (t, a, b, n, s, m, -1, 0)
    return H


_lists = {}


def hit_lists(key, hs, rays):
    """[H of rays[i]], computed once per key."""
    if key not in _lists:
        g = Geometry(hs)
        _lists[key] = [hit_list(g, r) for r in rays]
    return _lists[key]


def after_filter(H, t, slot):
    """The entries of H past the resume key (t, slot), by the header's comparison."""
    return H[(H["t"] > t) | ((H["t"] == t) & (H["slot"] > slot))]


def rows(lists, k):
    """What rt_trace_hits writes for these lists: ([n, k] HIT_DTYPE rows, count uint32 [n])."""
    out = np.full((len(lists), k), MISS, HIT_DTYPE)
    cnt = np.zeros(len(lists), np.uint32)
    for i, H in enumerate(lists):
        c = min(len(H), k)
        out[i, :c] = H[:c]
        cnt[i] = c
    return out, cnt


def raw(x):
    """Rows (HIT_DTYPE, or the float64 words of a result buffer) as int64 words: a bit-for-bit compare."""
    return np.ascontiguousarray(x).view(np.int64).reshape(-1, 8)
