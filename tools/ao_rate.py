"""Occlusion-fan rates (dev tool, needs the MI355X): rt_trace_ao against the same fan rays written out
and pushed through rt_trace_occluded, on the office proxy.
The points are the hit points of the 1920x1080 camera in tile-major order (rtamd.tile_major),
subsampled with a fixed stride to N points (default 131072), so that the materialised fan of the
larger k fits in memory (N k rays of 64 B).  For k in {16, 64} and two radii -- unbounded ("inf": the
office is a closed room, so every such ray is blocked and stops at its first hit) and half the
diagonal of the scene's box ("half": partly open fans) -- with cosine-weighted direction sets
(rtamd.ao_directions, 64 sets) and bias 1e-6:
  fused         rt_trace_ao on the N points;
  materialised  rt_trace_occluded on the N k fan rays of rtamd.ao_rays_host, written out once and
                uploaded, both untimed;
  sum           the per-point sum of the N k result bytes the caller then needs (a torch reduction);
  materialised_end_to_end   the two together.
Before anything is timed the fused counts are checked to equal k minus the materialised sums.
Each case is timed with HIP events over REPS launches (at least 20, default 50) after warm-up, in 5
interleaved rounds: median and [min, max] of the rounds, ms per launch.  No rate carries a pass
threshold.  RTAMD_HIP_LIB selects the library (A/B).

usage: python tools/ao_rate.py [REPS [N]]
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

REPS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 50
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 17
ROUNDS = 5
WARM = 5
W, H = 1920, 1080
KS = (16, 64)
N_SETS, SEED, BIAS = 64, 1, 1e-6
hs = rtamd.HostScene.generate("office")
hs.prepare()
dev = rtamd.DeviceScene(hs, 0)
lib = rtamd.hip_lib()


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


cam = torch.from_numpy(rtamd.camera_rays(hs.render_params(W, H, 1))[rtamd.tile_major(W, H)]).cuda()
hits = dev.trace(cam)
pts = rtamd.ao_points_from_hits(cam, hits)[torch.isfinite(hits["t"])]
n_hits = len(pts)
pts = pts[::max(1, n_hits // N)][:N].contiguous()
n = len(pts)

lo, hi = dev.bounds()
RADII = {"inf": float("inf"), "half": 0.5 * float(np.sqrt(((hi - lo) ** 2).sum()))}
cases, keep, open_fraction = {}, [], {}
for rname, radius in RADII.items():
    rpts = pts.clone()
    rpts[:, 6] = radius
    rpts_host = rpts.cpu().numpy()
    for k in KS:
        dirs_host = rtamd.ao_directions(k, N_SETS, seed=k)
        dirs = torch.from_numpy(dirs_host).cuda()
        fan = torch.from_numpy(rtamd.ao_rays_host(rpts_host, dirs_host, SEED, BIAS)).cuda()   # untimed
        a = abi.AoParams(k=k, n_sets=N_SETS, seed=SEED, bias=BIAS, d_dirs=dirs.data_ptr())
        counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
        occ = torch.zeros((n * k,), dtype=torch.uint8, device="cuda")
        sums = torch.zeros((n,), dtype=torch.int32, device="cuda")
        keep += [rpts, dirs, fan, a, counts, occ, sums]

        def fused(a=a, counts=counts, rpts=rpts):
            ok(lib.rt_trace_ao(dev._h, rpts.data_ptr(), n, C.byref(a), counts.data_ptr(), None, None))

        def materialised(fan=fan, occ=occ):
            ok(lib.rt_trace_occluded(dev._h, fan.data_ptr(), len(fan), occ.data_ptr(), None, None))

        def summed(occ=occ, sums=sums, k=k):
            torch.sum(occ.view(n, k), dim=1, dtype=torch.int32, out=sums)

        fused()
        materialised()
        summed()
        torch.cuda.synchronize()
        assert bool((counts == k - sums).all()), (rname, k)   # equal before anything is timed
        tag = f"{rname}_k{k}"
        open_fraction[tag] = round(float(counts.sum()) / (n * k), 4)
        cases[f"{tag}_fused"] = fused
        cases[f"{tag}_materialised"] = materialised
        cases[f"{tag}_sum"] = summed
        cases[f"{tag}_materialised_end_to_end"] = lambda m=materialised, s=summed: (m(), s())

runs = {c: [] for c in cases}
for _ in range(ROUNDS):   # the cases interleaved, so a drift of the machine shows as spread, not as a difference
    for c, call in cases.items():
        runs[c].append(timed(call))
res = {"workload": f"office_proxy: {n} of the {n_hits} hit points of the {W}x{H} camera, k in {list(KS)}, "
                   f"{N_SETS} cosine direction sets, radius inf and half the box diagonal ({RADII['half']:.4g})",
       "points": n, "fan_bytes": {f"k{k}": n * k * 64 for k in KS}, "result_bytes_fused": 4 * n,
       "open_fraction": open_fraction,
       "reps": REPS, "rounds": ROUNDS, "lib": os.environ.get("RTAMD_HIP_LIB", "in-tree"),
       "ms": {c: round(statistics.median(v), 4) for c, v in runs.items()},
       "ms_min_max": {c: [round(min(v), 4), round(max(v), 4)] for c, v in runs.items()}}
assert dev.status() == 0
print(json.dumps(res), flush=True)
