"""Ray-order rates (dev tool, needs the MI355X): what sorting incoherent rays with rt_ray_order buys
rt_trace_closest, rt_trace_occluded and rt_trace_radiance on the office proxy.
For each of the three calls, on the 1920x1080 camera rays (radiance: the scene's lights,
max_depth = 5, fp32 colours):
  (a) the rays in tile-major order (rtamd.tile_major: the render's 8x8 work tiles);
  (b) the same rays in a fixed random permutation;
  (d) the rays of (b) through the feature, for origin_bits 0 and -1: rt_ray_order, the gather of the
      rays, the call on the sorted rays and the scatter of its result rows, each alone, and all four
      end to end.
One more case has many origins: occlusion rays from (a)'s hit points to the first light, shuffled,
(b) and (d) as above.  Before anything is timed, (d)'s results are checked to equal (b)'s bit for
bit.  Each case is timed with HIP events over REPS launches (at least 20, default 50) after warm-up,
in 5 interleaved rounds: median and [min, max] of the rounds, ms per launch.  No rate carries a pass
threshold.  RTAMD_HIP_LIB selects the library (A/B).

usage: python tools/order_rate.py [REPS]
"""
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "my-raytracer_amd"))
import rtamd  # noqa: E402

REPS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 50
ROUNDS = 5
WARM = 5
W, H = 1920, 1080
hs = rtamd.HostScene.generate("office")
hs.prepare()
dev = rtamd.DeviceScene(hs, 0)
lib = rtamd.hip_lib()
p = hs.render_params(W, H, 1)
p.max_depth = 5
p.out_format = rtamd.RT_OUT_RGB_F32
p.flags = rtamd.abi.RT_FLAG_NATURAL_ORDER


def timed(call):
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS   # ms per launch


def ok(rc):
    assert rc == 0, lib.rt_last_error()


# the three calls over the C ABI: (rays, result rows) -> launch
def closest(rays, out):
    return lambda: ok(lib.rt_trace_closest(dev._h, rays.data_ptr(), len(rays), out.data_ptr(), None, None))


def occluded(rays, out):
    return lambda: ok(lib.rt_trace_occluded(dev._h, rays.data_ptr(), len(rays), out.data_ptr(), None, None))


def radiance(rays, out):
    return lambda: ok(lib.rt_trace_radiance(dev._h, C.byref(p), rays.data_ptr(), len(rays), out.data_ptr(), None, None))


def rows(kind, n):
    shape, dtype = {"closest": ((n, 8), torch.float64), "occluded": ((n,), torch.uint8),
                    "radiance": ((n, 3), torch.float32)}[kind]
    return torch.zeros(shape, dtype=dtype, device="cuda")


def permute(src, dst, perm, inverse):
    nbytes = (src.shape[1] if src.dim() == 2 else 1) * src.element_size()
    return lambda: ok(lib.rt_permute_rows(src.data_ptr(), dst.data_ptr(), perm.data_ptr(), len(src), nbytes,
                                          1 if inverse else 0, 0, None))


def order(rays, ob, perm, work):
    return lambda: ok(lib.rt_ray_order(dev._h, rays.data_ptr(), len(rays), ob, perm.data_ptr(), None, work.data_ptr(), None))


CALLS = {"closest": closest, "occluded": occluded, "radiance": radiance}
cases = {}   # name -> launch


def add_feature(tag, kind, rays_b, want_b):
    """(d) for the shuffled rays rays_b of one call: checked against want_b, then registered."""
    n = len(rays_b)
    for ob in (0, -1):
        perm = torch.zeros((n,), dtype=torch.int32, device="cuda")
        work = torch.zeros((rtamd.order_workspace_bytes(n),), dtype=torch.uint8, device="cuda")
        sorted_rays, sorted_out, out = torch.zeros_like(rays_b), rows(kind, n), rows(kind, n)
        steps = [order(rays_b, ob, perm, work), permute(rays_b, sorted_rays, perm, False),
                 CALLS[kind](sorted_rays, sorted_out), permute(sorted_out, out, perm, True)]
        for s in steps:
            s()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want_b.cpu().numpy().tobytes(), (tag, ob)
        pre = f"{tag}_d_ob{ob}"
        for name, s in zip(("order", "gather", "traced_sorted", "scatter"), steps):
            cases[f"{pre}_{name}"] = s
        cases[f"{pre}_end_to_end"] = lambda steps=steps: [s() for s in steps]


tile = rtamd.tile_major(W, H)
cam = rtamd.camera_rays(p)[tile]
rays_a = torch.from_numpy(cam).cuda()
shuffle = torch.from_numpy(np.random.default_rng(1).permutation(len(cam))).cuda()
rays_b = rays_a[shuffle].contiguous()
hits_a = None
for kind, call in CALLS.items():
    out_a, out_b = rows(kind, len(cam)), rows(kind, len(cam))
    call(rays_a, out_a)()
    call(rays_b, out_b)()
    torch.cuda.synchronize()
    assert out_b.cpu().numpy().tobytes() == out_a[shuffle].contiguous().cpu().numpy().tobytes(), kind
    if kind == "closest":
        hits_a = out_a.cpu().numpy()
    cases[f"{kind}_a_tile_major"] = call(rays_a, out_a)
    cases[f"{kind}_b_shuffled"] = call(rays_b, out_b)
    add_feature(kind, kind, rays_b, out_b)

# many origins: from (a)'s hit points to the first light, shuffled
hit = np.isfinite(hits_a[:, 0])
d = cam[hit, 3:6]
d = d / np.sqrt((d * d).sum(axis=1))[:, None]
pts = cam[hit, 0:3] + hits_a[hit, 0:1] * d
to_light = np.array(p.lights[0].position[:]) - pts
shadow = np.zeros((len(pts), 8))
shadow[:, 0:3], shadow[:, 3:6], shadow[:, 6] = pts, to_light, np.sqrt((to_light * to_light).sum(axis=1))
shadow = torch.from_numpy(shadow[np.random.default_rng(2).permutation(len(shadow))]).cuda()
occ_b = rows("occluded", len(shadow))
occluded(shadow, occ_b)()
torch.cuda.synchronize()
cases["shadow_b_shuffled"] = occluded(shadow, occ_b)
add_feature("shadow", "occluded", shadow, occ_b)

runs = {k: [] for k in cases}
for _ in range(ROUNDS):   # the cases interleaved, so a drift of the machine shows as spread, not as a difference
    for k, call in cases.items():
        runs[k].append(timed(call))
res = {"workload": f"office_proxy {W}x{H} camera rays ({len(cam)}), and {len(shadow)} shadow rays from their hit points",
       "reps": REPS, "rounds": ROUNDS, "lib": os.environ.get("RTAMD_HIP_LIB", "in-tree"),
       "ms": {k: round(statistics.median(v), 4) for k, v in runs.items()},
       "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in runs.items()}}
assert dev.status() == 0
print(json.dumps(res), flush=True)
