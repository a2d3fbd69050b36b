"""The numpy restatement of the camera's rays and surface points (csrc/device/rt_camera_point.hpp,
DESIGN.md §22) and the shards shared by tests/test_camera_abi.py and tests/test_camera_gpu.py.

numpy_rays and numpy_points restate rt_camera_rays_host and rt_surface_points_host operation by
operation in fp64 (numpy neither contracts nor reassociates), so the comparisons are bit for bit."""
import numpy as np

import rtamd
from ao_cases import same_bits  # noqa: F401  (bit equality, any NaN standing for any NaN)

ORDERS = ("row", "tile")
CAMERAS = [(32, 24), (13, 11), (9, 1), (1, 9), (1, 1), (8, 8)]

# shards of a 32 x 24 frame: name -> fields of rt_render_params.  "range_sh3" combines a row range
# whose row_begin is no multiple of stripe_height with that stripe height (stripe_count 1: the render
# launch refuses a row range with stripe_count > 1, and so does the camera call -- SHARD_REFUSED)
SHARDS = {
    "full": {},
    "range": dict(row_begin=5, row_end=17),
    "stripe0": dict(stripe_height=3, stripe_count=2, stripe_index=0),
    "stripe1": dict(stripe_height=3, stripe_count=2, stripe_index=1),
    "range_sh3": dict(row_begin=5, row_end=17, stripe_height=3, stripe_count=1, stripe_index=0),
}
SHARD_REFUSED = dict(row_begin=5, row_end=17, stripe_height=3, stripe_count=2, stripe_index=1)


def params(hs, W, H, **shard):
    p = hs.render_params(W, H, 1)
    for k, v in shard.items():
        setattr(p, k, v)
    return p


def shard_rows(p):
    """The shard's global rows, in packed order."""
    H = p.camera.height
    rb = max(0, p.row_begin)
    re = H if (p.row_end <= 0 or p.row_end > H) else p.row_end
    sh, sc, si = max(1, p.stripe_height), max(1, p.stripe_count), p.stripe_index
    return [y for y in range(H) if rb <= y < re and (y // sh) % sc == si]


def numpy_rays(p, order="row"):
    """rt_camera_rays_host in numpy: [rows * W, 8]."""
    cam = p.camera
    W = cam.width
    ys = shard_rows(p)
    eye, ll = np.array(cam.eye[:]), np.array(cam.lower_left[:])
    xd, yd = np.array(cam.x_dir[:]), np.array(cam.y_dir[:])
    X = np.arange(W, dtype=np.float64)[None, :]
    Y = np.array(ys, dtype=np.float64).reshape(-1, 1)
    rays = np.zeros((len(ys), W, 8))
    for c in range(3):
        rays[:, :, c] = eye[c]
        rays[:, :, 3 + c] = ((ll[c] + X * xd[c]) + Y * yd[c]) - eye[c]
    rays[:, :, 6] = np.inf
    rays = rays.reshape(len(ys) * W, 8)
    return rays[rtamd.tile_major(W, len(ys))] if order == "tile" else rays


def numpy_points(rays, hits_rows, point_tmax=np.inf):
    """rt_surface_points_host in numpy; the dot products in scalar order, left to right."""
    o, d = rays[:, 0:3], rays[:, 3:6]
    t, nrm = hits_rows[:, 0], hits_rows[:, 3:6]
    with np.errstate(all="ignore"):
        hit = t < np.inf
        ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        flip = nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1] + nrm[:, 2] * d[:, 2] > 0.0
        pts = np.zeros((len(rays), 8))
        for c in range(3):
            rd = np.where(ln > 0.0, d[:, c] / ln, d[:, c])
            pts[:, c] = np.where(hit, o[:, c] + t * rd, o[:, c])
            pts[:, 3 + c] = np.where(hit, np.where(flip, -nrm[:, c], nrm[:, c]), 0.0)
    pts[:, 6] = point_tmax
    return pts


def flipped(rays, hits_rows):
    """Hits whose normal the surface point turns round (numpy_points' rule)."""
    d, nrm = rays[:, 3:6], hits_rows[:, 3:6]
    return (hits_rows[:, 0] < np.inf) & (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1] + nrm[:, 2] * d[:, 2] > 0.0)


def synthetic(seed=17):
    """Ray and rt_hit rows for the host function: hits and misses, normals facing both ways, a dot
    product of exactly 0, zero normals, -0.0 components, directions of length 1e-150 and 1e150."""
    rng = np.random.default_rng(seed)
    n = 2048
    rays = np.zeros((n, 8))
    rays[:, 0:3] = rng.normal(size=(n, 3)) * 3.0
    rays[:, 3:6] = rng.normal(size=(n, 3))
    rays[:, 6] = np.inf
    hits = np.zeros((n, 8))
    hits[:, 0] = np.where(rng.random(n) < 0.3, np.inf, rng.random(n) * 10.0 + 1e-3)
    hits[:, 1:3] = rng.random((n, 2)) * 0.5
    hits[:, 3:6] = rng.normal(size=(n, 3))
    ints = hits.view(np.int32).reshape(n, 16)
    ints[:, 12:15] = -1
    hits[:, 0][:64] = rng.random(64) * 5.0 + 0.1   # the special rows below all hit
    # exactly perpendicular: d = (1, 0, 0), normal in the y-z plane -> dot == 0, not flipped
    rays[0:8, 3:6] = [1.0, 0.0, 0.0]
    hits[0:8, 3] = 0.0
    # ... and with -0.0 components on both sides
    rays[8:16, 3:6] = [-0.0, 2.0, -0.0]
    hits[8:16, 3:6] = [1.0, -0.0, -3.0]
    hits[16:24, 3:6] = 0.0                     # zero normals
    hits[24:28, 3:6] = [-0.0, -0.0, -0.0]
    rays[28:36, 0:3] *= 0.0                    # origins at +-0
    rays[28:32, 0:3] = -0.0
    for lo, hi, ln in ((36, 48, 1e-150), (48, 60, 1e150)):
        v = rays[lo:hi, 3:6]
        rays[lo:hi, 3:6] = v * (ln / np.sqrt((v * v).sum(1, keepdims=True)))
    return rays, hits
