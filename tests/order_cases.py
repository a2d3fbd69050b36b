"""Helpers shared by tests/test_order_abi.py and tests/test_order_gpu.py: the numpy restatement of
the ray coherence key (include/rt_hip.h) and the ray sets the key is checked on.

numpy_keys is written from the definition, not from the C++ text: fp64 throughout, + - * /, abs,
floor, comparisons and selects, so it gives the library's bits."""
import numpy as np

DEGENERATE = np.uint32(0x80000000)
ORIGIN_BITS = list(range(-1, 11))


def dir_bits(ob):
    return min(15, (31 - 3 * ob) // 2)


def _spread(x, step):
    """bit i of x -> bit step * i"""
    x = x.astype(np.uint64)
    out = np.zeros_like(x)
    for i in range(16):
        out |= ((x >> np.uint64(i)) & np.uint64(1)) << np.uint64(step * i)
    return out


def _cell(u, scale):
    c = np.floor(u * scale)
    c = np.where(c >= 0.0, c, 0.0)
    c = np.where(c > scale - 1.0, scale - 1.0, c)
    return c.astype(np.uint64)


def numpy_keys(lo, hi, rays, origin_bits=-1):
    """uint32 [n]: the key of every ray ([n, 8] float64 rows: o, d, tmax, reserved) in box [lo, hi]."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    rays = np.asarray(rays, np.float64)
    ob = 5 if origin_bits < 0 else origin_bits
    db = dir_bits(ob)
    o, d, tmax = rays[:, 0:3], rays[:, 3:6], rays[:, 6]
    with np.errstate(all="ignore"):
        dd = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        act = np.all(np.abs(o) <= np.finfo(np.float64).max, axis=1) & np.all(np.abs(d) <= np.finfo(np.float64).max, axis=1)
        act &= (dd > 0.0) & (tmax > 1e-5)
        mo = np.zeros(len(rays), np.uint64)
        for k in range(3):
            e = hi[k] - lo[k]
            c = _cell((o[:, k] - lo[k]) / e, float(1 << ob)) if e > 0.0 else np.zeros(len(rays), np.uint64)
            mo |= _spread(c, 3) << np.uint64(k)
        s = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
        px, py = d[:, 0] / s, d[:, 1] / s
        fx = (1.0 - np.abs(py)) * np.where(px >= 0.0, 1.0, -1.0)
        fy = (1.0 - np.abs(px)) * np.where(py >= 0.0, 1.0, -1.0)
        neg = d[:, 2] < 0.0
        px, py = np.where(neg, fx, px), np.where(neg, fy, py)
        qu = _cell(px * 0.5 + 0.5, float(1 << db))
        qv = _cell(py * 0.5 + 0.5, float(1 << db))
    md = _spread(qu, 2) | (_spread(qv, 2) << np.uint64(1))
    key = (mo << np.uint64(2 * db)) | md
    assert np.all(key[act] < (1 << 31))
    return np.where(act, key, np.uint64(DEGENERATE)).astype(np.uint32)


def make_rays(o, d, tmax=np.inf):
    o, d = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
    n = max(len(o), len(d))
    rays = np.zeros((n, 8))
    rays[:, 0:3] = o
    rays[:, 3:6] = d
    rays[:, 6] = tmax
    return rays


def box_rays(lo, hi, n=4096, seed=11):
    """Random rays around a box: origins in the box widened by a quarter, normal directions."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    return make_rays(lo - 0.25 * ext + rng.random((n, 3)) * 1.5 * ext, rng.normal(size=(n, 3)))


def special_directions():
    """The six axis directions, the twelve face diagonals, dz = +0.0 and -0.0."""
    d = []
    for k in range(3):
        for s in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]
            v[k] = s
            d.append(v)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                v = [0.0, 0.0, 0.0]
                v[a], v[b] = sa, sb
                d.append(v)
    d += [[0.3, -0.7, 0.0], [0.3, -0.7, -0.0], [-1.0, 0.0, -0.0], [0.0, 0.0, -1.0]]
    return np.array(d)


def extreme_rays(lo, hi):
    """Origins on the hi faces, far outside and inside; tiny and huge components."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    mid = 0.5 * (lo + hi)
    o = [hi, lo, mid, [hi[0], mid[1], mid[2]], [mid[0], hi[1], mid[2]], [mid[0], mid[1], hi[2]],
         [1e300, -1e300, 1e300], [-1e300, 1e300, -1e300], [1e-310, -1e-310, 1e-310], np.nextafter(hi, -np.inf),
         np.nextafter(hi, np.inf), np.nextafter(lo, -np.inf)]
    d = [[1e-310, 1.0, -1.0], [1e300, 1e300, -1e300], [1e300, 1e-310, 1e-310], [-1e-310, -1e300, 1.0],
         [1.0, 2.0, 3.0], [-3.0, 2.0, -1.0], [1.7e308, 1.7e308, 1.7e308], [1e-150, 1e-150, -1e-150]]
    rays = [make_rays(oi, di) for oi in o for di in d]
    return np.concatenate(rays)


def degenerate_rays():
    """One ray of each degenerate kind (the queries' rule): all get DEGENERATE."""
    base = make_rays([0.1, 0.2, 0.3], [1.0, 2.0, 3.0])
    out = []
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            r = base.copy()
            r[0, k] = bad
            out.append(r)
    for d in ([0.0, 0.0, 0.0], [1e-310, 1e-310, 1e-310], [-0.0, 0.0, 1e-170]):
        out.append(make_rays([0.1, 0.2, 0.3], d))
    for tmax in (np.nan, 1e-5, 0.0, -1.0, -np.inf):
        out.append(make_rays([0.1, 0.2, 0.3], [1.0, 2.0, 3.0], tmax))
    return np.concatenate(out)


def pinhole_rays(width, height, fov_deg=60.0):
    """Rays of a pinhole camera at the origin looking down -z, row-major."""
    t = np.tan(np.radians(fov_deg) / 2.0)
    x = ((np.arange(width) + 0.5) / width * 2.0 - 1.0) * t * width / height
    y = ((np.arange(height) + 0.5) / height * 2.0 - 1.0) * t
    xs, ys = np.meshgrid(x, y)
    d = np.stack([xs.ravel(), ys.ravel(), -np.ones(width * height)], axis=1)
    return make_rays(np.zeros(3), d)


def mean_wave_bbox(order, width, wave=64):
    """Mean pixel bounding-box area of each `wave` consecutive entries of order (pixel ids y * width + x)."""
    order = np.asarray(order)
    areas = []
    for i in range(0, len(order), wave):
        p = order[i:i + wave]
        x, y = p % width, p // width
        areas.append((x.max() - x.min() + 1) * (y.max() - y.min() + 1))
    return float(np.mean(areas))
