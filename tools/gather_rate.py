"""Fan-gather rates (dev tool, needs the MI355X): rt_trace_gather against the same fan rays written out,
shaded by rt_trace_radiance and reduced per point by the caller, on the office proxy.
The points are the hit points of the 1920x1080 camera in tile-major order (rtamd.tile_major),
subsampled with a fixed stride to N points (default 131072), so that the written-out fan of the
larger k fits in memory (N k rays of 64 B and N k colours of 24 B).  For k in {16, 64} and two radii
-- unbounded ("inf") and half the diagonal of the scene's box ("half") -- with cosine-weighted
direction sets (rtamd.ao_directions, 64 sets), bias 1e-6, the scene's own lights and max_depth,
fp64 output:
  fused         rt_trace_gather on the N points;
  written_out   rt_trace_radiance on the N k fan rays of rtamd.ao_rays_host, written out once and
                uploaded, both untimed;
  mean          the per-point mean of the N k colours the caller then needs (a torch reduction:
                torch.sum over the sample axis and one division; its order is torch's, not the
                sample order, so it is the cost of such a reduction and not the reference);
  written_out_end_to_end   the two together.
Before anything is timed the fused result is checked to equal, bit for bit, the written-out colours
summed in sample order (a loop of k torch additions) and divided by k.
Each case is timed with HIP events over REPS launches (at least 5, default 20) after warm-up, in 5
interleaved rounds: median and [min, max] of the rounds, ms per launch.  No rate carries a pass
threshold.  RTAMD_HIP_LIB selects the library (A/B).

usage: python tools/gather_rate.py [REPS [N]]
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
from rtamd import abi  # noqa: E402

REPS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 20
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 17
ROUNDS = 5
WARM = 2
W, H = 1920, 1080
KS = (16, 64)
N_SETS, SEED, BIAS = 64, 1, 1e-6
hs = rtamd.HostScene.generate("office")
hs.prepare()
dev = rtamd.DeviceScene(hs, 0)
lib = rtamd.hip_lib()
params = hs.render_params(W, H, 1)
params.out_format = rtamd.RT_OUT_RGB_F64


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


cam = torch.from_numpy(rtamd.camera_rays(params)[rtamd.tile_major(W, H)]).cuda()
hits = dev.trace(cam)
pts = rtamd.ao_points_from_hits(cam, hits)[torch.isfinite(hits["t"])]
n_hits = len(pts)
pts = pts[::max(1, n_hits // N)][:N].contiguous()
n = len(pts)
del cam, hits

lo, hi = dev.bounds()
RADII = {"inf": float("inf"), "half": 0.5 * float(np.sqrt(((hi - lo) ** 2).sum()))}
cases, keep, mean_colour, rays_traced = {}, [], {}, {}
for rname, radius in RADII.items():
    rpts = pts.clone()
    rpts[:, 6] = radius
    rpts_host = rpts.cpu().numpy()
    for k in KS:
        dirs_host = rtamd.ao_directions(k, N_SETS, seed=k)
        dirs = torch.from_numpy(dirs_host).cuda()
        fan = torch.from_numpy(rtamd.ao_rays_host(rpts_host, dirs_host, SEED, BIAS)).cuda()   # untimed
        a = abi.AoParams(k=k, n_sets=N_SETS, seed=SEED, bias=BIAS, d_dirs=dirs.data_ptr())
        rgb = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        cols = torch.zeros((n * k, 3), dtype=torch.float64, device="cuda")
        means = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        keep += [rpts, dirs, fan, a, rgb, cols, means]

        def fused(a=a, rgb=rgb, rpts=rpts, stats=None):
            ok(lib.rt_trace_gather(dev._h, C.byref(params), rpts.data_ptr(), n, C.byref(a), rgb.data_ptr(), stats, None))

        def written_out(fan=fan, cols=cols, stats=None):
            ok(lib.rt_trace_radiance(dev._h, C.byref(params), fan.data_ptr(), len(fan), cols.data_ptr(), stats, None))

        def mean(cols=cols, means=means, k=k):
            torch.sum(cols.view(n, k, 3), dim=1, out=means)
            means.div_(float(k))

        sf, sw = abi.Stats(), abi.Stats()
        fused(stats=C.byref(sf))
        written_out(stats=C.byref(sw))
        acc = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        for s in range(k):   # in sample order, one addition per sample
            acc = acc + cols.view(n, k, 3)[:, s, :]
        torch.cuda.synchronize()
        assert bool((rgb == acc / float(k)).all()), (rname, k)   # equal before anything is timed
        counts = [int(sf.primary_rays), int(sf.shadow_rays), int(sf.reflection_rays)]
        assert counts == [int(sw.primary_rays), int(sw.shadow_rays), int(sw.reflection_rays)], (rname, k)
        del acc
        tag = f"{rname}_k{k}"
        mean_colour[tag] = [round(float(v), 4) for v in rgb.mean(dim=0)]
        rays_traced[tag] = counts
        cases[f"{tag}_fused"] = fused
        cases[f"{tag}_written_out"] = written_out
        cases[f"{tag}_mean"] = mean
        cases[f"{tag}_written_out_end_to_end"] = lambda m=written_out, s=mean: (m(), s())

runs = {c: [] for c in cases}
for _ in range(ROUNDS):   # the cases interleaved, so a drift of the machine shows as spread, not as a difference
    for c, call in cases.items():
        runs[c].append(timed(call))
res = {"workload": f"office_proxy: {n} of the {n_hits} hit points of the {W}x{H} camera, k in {list(KS)}, "
                   f"{N_SETS} cosine direction sets, radius inf and half the box diagonal ({RADII['half']:.4g}), "
                   f"{params.n_lights} lights, max_depth {params.max_depth}, fp64 colours",
       "points": n, "fan_bytes": {f"k{k}": n * k * 64 for k in KS}, "colour_bytes": {f"k{k}": n * k * 24 for k in KS},
       "result_bytes_fused": 24 * n, "mean_colour": mean_colour, "rays_primary_shadow_reflection": rays_traced,
       "reps": REPS, "rounds": ROUNDS, "lib": os.environ.get("RTAMD_HIP_LIB", "in-tree"),
       "ms": {c: round(statistics.median(v), 4) for c, v in runs.items()},
       "ms_min_max": {c: [round(min(v), 4), round(max(v), 4)] for c, v in runs.items()}}
assert dev.status() == 0
print(json.dumps(res), flush=True)
