"""Inputs and the numpy restatement of the occlusion fan (csrc/device/rt_ao_fan.hpp)
shared by tests/test_ao_abi.py and tests/test_ao_gpu.py.

numpy_rays restates rt_ao_rays_host operation by operation in fp64 (numpy neither contracts nor
reassociates), so the comparison with the library is bit for bit."""
import numpy as np

K_MAX, SETS_MAX = 1024, 65536


def numpy_hash(x):
    """rt_ao_hash on a uint32 array."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def numpy_sets(n, seed, n_sets):
    """The direction set of points 0..n-1."""
    i = np.arange(n, dtype=np.uint64).astype(np.uint32)
    return numpy_hash(i ^ np.uint32(seed)) % np.uint32(n_sets)


def numpy_valid(points):
    o, d, tmax = points[:, 0:3], points[:, 3:6], points[:, 6]
    with np.errstate(all="ignore"):
        dd = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        fin = np.all(np.abs(o) <= np.finfo(np.float64).max, axis=1) & np.all(np.abs(d) <= np.finfo(np.float64).max, axis=1)
        return fin & (dd > 0.0) & (tmax > 1e-5)


def numpy_frame(nrm):
    """(N, T, B) of normals [n, 3], in the header's operations and association."""
    with np.errstate(all="ignore"):
        x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
        ln = np.sqrt(x * x + y * y + z * z)
        nx, ny, nz = x / ln, y / ln, z / ln
        sg = np.where(nz >= 0.0, 1.0, -1.0)
        a = -1.0 / (sg + nz)
        b = nx * ny * a
        T = np.stack([1.0 + sg * nx * nx * a, sg * b, -sg * nx], 1)
        B = np.stack([b, sg + ny * ny * a, -ny], 1)
        return np.stack([nx, ny, nz], 1), T, B


def numpy_rays(points, dirs, seed, bias):
    """rt_ao_rays_host in numpy: [n * k, 8] rays."""
    points = np.asarray(points, dtype=np.float64)
    n, (n_sets, k) = len(points), dirs.shape[:2]
    valid = numpy_valid(points)
    N, T, B = numpy_frame(points[:, 3:6])
    l = dirs[numpy_sets(n, seed, n_sets).astype(np.int64)]   # [n, k, 3]
    rays = np.zeros((n, k, 8))
    with np.errstate(all="ignore"):
        for c in range(3):
            w = (l[:, :, 0] * T[:, None, c] + l[:, :, 1] * B[:, None, c]) + l[:, :, 2] * N[:, None, c]
            rays[:, :, 3 + c] = np.where(valid[:, None], w, 0.0)
            rays[:, :, c] = np.where(valid, points[:, c] + bias * N[:, c], points[:, c])[:, None]
    rays[:, :, 6] = points[:, 6][:, None]
    return rays.reshape(n * k, 8)


def same_bits(a, b):
    """Equal bit for bit, any NaN standing for any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def make_points(p, nrm, tmax=np.inf):
    pts = np.zeros((len(p), 8))
    pts[:, 0:3] = p
    pts[:, 3:6] = nrm
    pts[:, 6] = tmax
    return pts


def special_normals():
    """Axis normals (N.z = -1 and -0.0 included) and the face diagonals: well scaled."""
    out = []
    for ax in range(3):
        for sgn in (1.0, -1.0):
            v = np.zeros(3)
            v[ax] = sgn
            out.append(v)
    out.append(np.array([1.0, 0.0, -0.0]))
    for a in (1.0, -1.0):
        for b in (1.0, -1.0):
            out += [np.array([a, b, 0.0]), np.array([a, 0.0, b]), np.array([0.0, a, b])]
    for a in (1.0, -1.0):
        for b in (1.0, -1.0):
            for c in (1.0, -1.0):
                out.append(np.array([a, b, c]))
    return np.array(out)


def degenerate_points():
    """Every kind of point the fan never traces."""
    good = make_points([[0.5, -0.25, 2.0]], [[0.3, -0.4, 0.8]], 3.0)[0]
    out = []
    for col, val in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, -np.inf),
                     (6, np.nan), (6, 0.0), (6, 1e-5), (6, -1.0)):
        r = good.copy()
        r[col] = val
        out.append(r)
    z = good.copy()
    z[3:6] = 0.0
    out.append(z)
    u = good.copy()
    u[3:6] = [1e-170, -1e-170, 1e-170]   # dot(d, d) underflows to 0
    out.append(u)
    return np.array(out)


def host_points(seed=11):
    """The point set the host function is pinned on: (well-scaled points, all points)."""
    rng = np.random.default_rng(seed)
    n = 4096
    rand = make_points(rng.normal(size=(n, 3)) * 3.0, rng.normal(size=(n, 3)),
                       np.where(rng.random(n) < 0.5, np.inf, rng.random(n) * 4.0 + 0.5))
    sn = special_normals()
    spec = make_points(rng.normal(size=(len(sn), 3)), sn)
    well = np.concatenate([rand, spec])
    tiny = make_points(rng.normal(size=(64, 3)), rng.normal(size=(64, 3)))
    tiny[:, 3:6] *= 1e-150 / np.sqrt((tiny[:, 3:6] ** 2).sum(1, keepdims=True))
    huge = make_points(rng.normal(size=(64, 3)), rng.normal(size=(64, 3)), 2.0)
    huge[:, 3:6] *= 1e150 / np.sqrt((huge[:, 3:6] ** 2).sum(1, keepdims=True))
    over = make_points(rng.normal(size=(4, 3)), rng.normal(size=(4, 3)) * 1e200)   # dot(d, d) overflows
    return well, np.concatenate([well, tiny, huge, over, degenerate_points(), spec[:5]])


def host_dirs(n_sets, k=12, seed=2):
    """Unit hemisphere directions with, in every set, a zero vector, zero components and a NaN."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_sets, k, 3))
    d[..., 2] = np.abs(d[..., 2])
    d /= np.sqrt((d * d).sum(2, keepdims=True))
    d[:, 0] = [0.0, 0.0, 0.0]
    d[:, 1] = [0.0, 0.0, 1.0]
    d[:, 2] = [1.0, 0.0, 0.0]
    d[:, 3] = [np.nan, 0.0, 1.0]
    d[:, 4] = [0.0, -0.0, -1.0]
    return d
