"""Ray-query rates (dev tool, needs the MI355X): rt_trace_closest / rt_trace_occluded on the office
proxy, beside the render kernel tracing the same primary rays.
  (a) the 1920x1080 camera rays in tile-major order (the render kernel's 8x8 work tiles);
  (b) the same rays in a fixed random permutation;
  (c) occlusion rays from (a)'s hit points to the first light;
  render: a primary-only launch of the same camera (n_lights = 0, max_depth = 0).
Each case is timed with HIP events over REPS launches (at least 20, default 200) after warm-up, in
5 interleaved rounds, and printed as Mrays/s (median, and [min, max] of the rounds).  The rates
carry no pass threshold.  RTAMD_HIP_LIB selects the library (A/B).

usage: python tools/query_rate.py [REPS]
"""
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

REPS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 200
ROUNDS = 5
WARM = 5
W, H = 1920, 1080
hs = rtamd.HostScene.generate("office")
hs.prepare()
dev = rtamd.DeviceScene(hs, 0)
p = hs.render_params(W, H, 1)

# camera rays, tile-major: the 64 rays of one tile are consecutive
tw, th = rtamd.tile_shape()
ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
key = ((ys // th) * ((W + tw - 1) // tw) + xs // tw) * (tw * th) + (ys % th) * tw + xs % tw
order = np.argsort(key.ravel(), kind="stable")
rays_a = torch.from_numpy(rtamd.camera_rays(p)[order]).cuda()
perm = torch.from_numpy(np.random.default_rng(1).permutation(W * H)).cuda()
rays_b = rays_a[perm].contiguous()
N = W * H


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


hits, st_a = dev.trace(rays_a, stats=True)
# (c): from each hit point towards the first light, bounded by the light distance
hit = torch.isfinite(hits["t"])
o, d = rays_a[hit, 0:3], rays_a[hit, 3:6]
dn = d / torch.sqrt((d * d).sum(1, keepdim=True))
pts = o + hits["t"][hit][:, None] * dn
light = torch.tensor(list(hs.raw.contents.lights[0].position[:]), dtype=torch.float64, device="cuda")
rays_c = torch.zeros((pts.shape[0], 8), dtype=torch.float64, device="cuda")
rays_c[:, 0:3] = pts
rays_c[:, 3:6] = light - pts
rays_c[:, 6] = torch.sqrt(((light - pts) ** 2).sum(1))
occ, st_c = dev.trace(rays_c, occluded=True, stats=True)

# the render kernel on the same camera, primary rays only
q = rtamd.abi.RenderParams.from_buffer_copy(p)
q.n_lights = 0
q.max_depth = 0
q.out_format = rtamd.RT_OUT_RGB_F32
d_out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
rst = dev.launch(q, d_out.data_ptr(), stats=True)
assert rst.primary_rays == N and rst.shadow_rays == 0 and rst.reflection_rays == 0

# the timed launches go straight to the C ABI with result buffers made once (DeviceScene.trace
# allocates and clears a new one per call)
lib = rtamd.hip_lib()
d_hits = torch.zeros((N, 8), dtype=torch.float64, device="cuda")
d_occ = torch.zeros((rays_c.shape[0],), dtype=torch.uint8, device="cuda")


def closest(rays):
    def f():
        assert lib.rt_trace_closest(dev._h, rays.data_ptr(), rays.shape[0], d_hits.data_ptr(), None, None) == 0
    return f


def occluded():
    assert lib.rt_trace_occluded(dev._h, rays_c.data_ptr(), rays_c.shape[0], d_occ.data_ptr(), None, None) == 0


cases = {"closest_tile_major": closest(rays_a), "closest_permuted": closest(rays_b), "occluded_to_light": occluded,
         "render_primary_only": lambda: dev.launch(q, d_out.data_ptr())}
counts = {"closest_tile_major": N, "closest_permuted": N, "occluded_to_light": int(rays_c.shape[0]),
          "render_primary_only": N}
runs = {k: [] for k in cases}
for _ in range(ROUNDS):   # the cases interleaved, so a drift of the machine shows as spread, not as a difference
    for k, call in cases.items():
        runs[k].append(timed(call))
ms = {k: statistics.median(v) for k, v in runs.items()}
res = {"workload": f"office_proxy {W}x{H} camera rays", "reps": REPS, "rounds": ROUNDS,
       "lib": os.environ.get("RTAMD_HIP_LIB", "in-tree"),
       "hits": int(st_a.hits), "occluded": int(st_c.hits), "stack_spills_closest": int(st_a.stack_spills),
       "ms": {k: round(v, 4) for k, v in ms.items()},
       "mrays_per_s": {k: round(counts[k] / ms[k] / 1e3, 1) for k in ms},
       "mrays_per_s_min_max": {k: [round(counts[k] / max(v) / 1e3, 1), round(counts[k] / min(v) / 1e3, 1)]
                               for k, v in runs.items()}}
assert dev.status() == 0
print(json.dumps(res), flush=True)
