"""Camera surface-point rates (dev tool, needs the MI355X): rt_trace_camera against the written-out
chain it replaces, on the office proxy at 1920x1080.  Both sides end with the frame's
surface-point records in tile-major order on the device, the input of rt_trace_ao / rt_trace_gather:
  fused        rt_trace_camera, points only, RT_CAMERA_TILE_MAJOR: nothing is read per pixel;
  written_out  the tile-major camera rays (rtamd.camera_rays_host, built and uploaded once, untimed),
               then rt_trace_closest on them and rtamd.ao_points_from_hits on rays and hits;
  closest      the rt_trace_closest call of that chain alone;
  points       the ao_points_from_hits step alone.
Before anything is timed the fused records are checked to equal, bit for bit, rt_surface_points_host
of the rays and rt_trace_closest's hits -- the written-out chain with the definition's own operation
order.  The torch step of the chain is compared too and its differences are reported, not asserted:
torch's reductions over the three components need not add in the header's order, so a record may
differ in the last bits of p (never in which way the normal faces, short of a dot product that rounds
across zero).  Each
case is timed with HIP events over REPS launches (at least 20, default 50) after warm-up, in 5
interleaved rounds: median and [min, max] of the rounds, ms per launch.  The bytes each side holds on
the device are printed too.  No rate carries a pass threshold.  RTAMD_HIP_LIB selects the library (A/B).

usage: python tools/camera_rate.py [REPS]
"""
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "my-raytracer_amd"))
import rtamd  # noqa: E402
from rtamd import abi  # noqa: E402

REPS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 50
ROUNDS = 5
WARM = 5
W, H = 1920, 1080
hs = rtamd.HostScene.generate("office")
hs.prepare()
dev = rtamd.DeviceScene(hs, 0)
lib = rtamd.hip_lib()
params = hs.render_params(W, H, 1)
n = W * H


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


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int64) == b.view(torch.int64)).all())


rays_host = rtamd.camera_rays_host(params, "tile")   # untimed
rays = torch.from_numpy(rays_host).cuda()
hit_rows = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
fused_pts = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
out = abi.CameraOut(d_hits=None, d_points=fused_pts.data_ptr(), order=abi.RT_CAMERA_TILE_MAJOR,
                    point_tmax=float("inf"))
chain = {}


def fused():
    ok(lib.rt_trace_camera(dev._h, C.byref(params), C.byref(out), None, None))


def closest():
    ok(lib.rt_trace_closest(dev._h, rays.data_ptr(), n, hit_rows.data_ptr(), None, None))


def points():
    chain["pts"] = rtamd.ao_points_from_hits(rays, rtamd._hit_views(hit_rows))


def written_out():
    closest()
    points()


# the two sides hold the same bits before anything is timed
fused()
torch.cuda.synchronize()
base = torch.cuda.memory_allocated()
torch.cuda.reset_peak_memory_stats()
written_out()
torch.cuda.synchronize()
chain_peak = torch.cuda.max_memory_allocated() - base   # the point records and the torch temporaries
want = torch.from_numpy(rtamd.surface_points_host(rays_host, hit_rows.cpu().numpy())).cuda()
assert same_bits(fused_pts, want), "rt_trace_camera differs from rt_surface_points_host of rt_trace_closest"
n_hit = int(torch.isfinite(hit_rows[:, 0]).sum())
diff = fused_pts.view(torch.int64) != chain["pts"].view(torch.int64)
scale = fused_pts[:, 0:3].abs().max()
torch_step = {"differing_records": int(diff.any(dim=1).sum()),
              "differing_records_by_column": [int(x) for x in diff.sum(dim=0)],
              "max_abs_difference_of_p": float((fused_pts[:, 0:3] - chain["pts"][:, 0:3]).abs().max()),
              "max_abs_p": float(scale)}
del want, diff

cases = {"fused": fused, "written_out": written_out, "closest": closest, "points": points}
runs = {c: [] for c in cases}
for _ in range(ROUNDS):   # the cases interleaved, so a drift of the machine shows as spread, not as a difference
    for c, call in cases.items():
        runs[c].append(timed(call))
res = {"workload": f"office_proxy {W}x{H}: {n} pixels, {n_hit} hit, surface points in tile-major order",
       "pixels": n, "hits": n_hit, "fused_equals_surface_points_host_of_trace_closest": True,
       "torch_step_against_fused": torch_step,
       "bytes_held": {"fused": {"points": 64 * n},
                      "written_out": {"rays": 64 * n, "hits": 64 * n, "points_and_torch_temporaries_peak": int(chain_peak)}},
       "reps": REPS, "rounds": ROUNDS, "lib": os.environ.get("RTAMD_HIP_LIB", "in-tree"),
       "ms": {c: round(statistics.median(v), 4) for c, v in runs.items()},
       "ms_min_max": {c: [round(min(v), 4), round(max(v), 4)] for c, v in runs.items()}}
assert dev.status() == 0
print(json.dumps(res), flush=True)
