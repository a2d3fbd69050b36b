"""Radiance rates (dev tool, needs the MI355X): rt_trace_radiance on the office proxy beside the frame
launch that shades the same rays, with the scene's lights and max_depth = 5.
  (a) the 1920x1080 camera rays in tile-major order (rtamd.tile_major: the render's 8x8 work tiles);
  (b) the same rays in a fixed random permutation;
  (c) the yardstick: a one-frame rt_launch_compute_image of the same params with
      RT_FLAG_NATURAL_ORDER.
All three write fp32 colours.  Each case is timed with HIP events over REPS launches (at least 20,
default 100) after warm-up, in 5 interleaved rounds, and printed as ms per launch and Mrays/s over
all ray kinds (primary + shadow + reflection, from the launch's stats): median, and [min, max] of
the rounds.  The rates carry no pass threshold.  RTAMD_HIP_LIB selects the library (A/B).

usage: python tools/radiance_rate.py [REPS]
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

REPS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 100
ROUNDS = 5
WARM = 5
W, H = 1920, 1080
N = W * H
hs = rtamd.HostScene.generate("office")
hs.prepare()
dev = rtamd.DeviceScene(hs, 0)
p = hs.render_params(W, H, 1)
p.max_depth = 5
p.out_format = rtamd.RT_OUT_RGB_F32
p.flags = rtamd.abi.RT_FLAG_NATURAL_ORDER

order = rtamd.tile_major(W, H)
rays_a = torch.from_numpy(rtamd.camera_rays(p)[order]).cuda()
perm = torch.from_numpy(np.random.default_rng(1).permutation(N)).cuda()
rays_b = rays_a[perm].contiguous()


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


# the timed launches go straight to the C ABI with result buffers made once
lib = rtamd.hip_lib()
d_rgb = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
d_out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")


def radiance(rays, stats=None):
    def f():
        assert lib.rt_trace_radiance(dev._h, C.byref(p), rays.data_ptr(), N, d_rgb.data_ptr(),
                                     C.byref(stats) if stats is not None else None, None) == 0
    return f


def all_rays(st):
    return int(st.primary_rays + st.shadow_rays + st.reflection_rays)


# ray counts of each case, and the three results agree: (a) and (b) un-permuted equal the frame
st_a, st_b = rtamd.abi.Stats(), rtamd.abi.Stats()
st_c = dev.launch(p, d_out.data_ptr(), stats=True)
frame = d_out.reshape(N, 3)[torch.from_numpy(order).cuda()].clone()
radiance(rays_a, st_a)()
assert bool((d_rgb == frame).all())
radiance(rays_b, st_b)()
assert bool((d_rgb == frame[perm]).all())
assert all_rays(st_a) == all_rays(st_b) == all_rays(st_c) and st_a.primary_rays == N

cases = {"radiance_tile_major": radiance(rays_a), "radiance_permuted": radiance(rays_b),
         "frame_natural_order": lambda: dev.launch(p, d_out.data_ptr())}
counts = {"radiance_tile_major": all_rays(st_a), "radiance_permuted": all_rays(st_b),
          "frame_natural_order": all_rays(st_c)}
runs = {k: [] for k in cases}
for _ in range(ROUNDS):   # the cases interleaved, so a drift of the machine shows as spread, not as a difference
    for k, call in cases.items():
        runs[k].append(timed(call))
ms = {k: statistics.median(v) for k, v in runs.items()}
res = {"workload": f"office_proxy {W}x{H} camera rays, scene lights, max_depth 5, fp32 out", "reps": REPS,
       "rounds": ROUNDS, "lib": os.environ.get("RTAMD_HIP_LIB", "in-tree"),
       "rays": {"primary": int(st_a.primary_rays), "shadow": int(st_a.shadow_rays),
                "reflection": int(st_a.reflection_rays)},
       "ms": {k: round(v, 4) for k, v in ms.items()},
       "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in runs.items()},
       "mrays_per_s": {k: round(counts[k] / ms[k] / 1e3, 1) for k in ms},
       "mrays_per_s_min_max": {k: [round(counts[k] / max(v) / 1e3, 1), round(counts[k] / min(v) / 1e3, 1)]
                               for k, v in runs.items()},
       "radiance_over_frame": round(ms["frame_natural_order"] / ms["radiance_tile_major"], 4)}
assert dev.status() == 0
print(json.dumps(res), flush=True)
