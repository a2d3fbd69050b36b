"""Hit-list rates (dev tool, needs the MI355X): rt_trace_hits beside rt_trace_closest and beside
what a caller could do before it, on two scenes:
  office: the office proxy, its 1920x1080 camera rays in tile-major order;
  random: the random-triangle scene (RANDOM_TRIS triangles), 2^20 rays with origins around its box
          and normal-distributed directions (long lists: tens of hits on many rays).
Per scene:
  closest          rt_trace_closest on the rays;
  hits_k1/2/4/8    rt_trace_hits with that k (no resume keys);
  all_hits_k8      DeviceScene.all_hits(k=8): resumed rounds, compaction and the CSR result;
  advance_k8       the old way to the same depth: 8 rounds of rt_trace_closest, each from the last
                   hit point pushed PUSH along the ray, with torch between the rounds; `lost` counts
                   the entries of the exact first-8 lists it misses, `extra` the entries it reports
                   that are not in them or are reported twice.
Each case is timed with HIP events over REPS launches (default 10) after warm-up, in 3 interleaved
rounds, and printed as Mrays/s (median, and [min, max] of the rounds).  The rates carry no pass
threshold.  RTAMD_HIP_LIB selects the library (A/B).

usage: python tools/hits_rate.py [REPS]
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

REPS = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 10
ROUNDS = 3
WARM = 2
W, H = 1920, 1080
RANDOM_TRIS = 100000
RANDOM_RAYS = 1 << 20
PUSH = 1e-4
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
    return e0.elapsed_time(e1) / REPS   # ms per call


def office():
    hs = rtamd.HostScene.generate("office")
    hs.prepare()
    p = hs.render_params(W, H, 1)
    tw, th = rtamd.tile_shape()
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    key = ((ys // th) * ((W + tw - 1) // tw) + xs // tw) * (tw * th) + (ys % th) * tw + xs % tw
    order = np.argsort(key.ravel(), kind="stable")
    return hs, torch.from_numpy(rtamd.camera_rays(p)[order]).cuda()


def random_scene():
    hs = rtamd.HostScene.generate("random_tris", n_triangles=RANDOM_TRIS)
    hs.prepare()
    b = hs.bvh_arrays()
    lo, hi = b["bb_min"][0], b["bb_max"][0]
    rng = np.random.default_rng(7)
    rays = np.zeros((RANDOM_RAYS, 8))
    rays[:, 0:3] = lo - 0.25 * (hi - lo) + rng.random((RANDOM_RAYS, 3)) * 1.5 * (hi - lo)
    rays[:, 3:6] = rng.normal(size=(RANDOM_RAYS, 3))
    rays[:, 6] = np.inf
    return hs, torch.from_numpy(rays).cuda()


def measure(name, hs, rays):
    dev = rtamd.DeviceScene(hs, 0)
    n = rays.shape[0]
    d_hits = torch.zeros((n * 8, 8), dtype=torch.float64, device="cuda")
    d_count = torch.zeros((n,), dtype=torch.int32, device="cuda")

    def closest(r=rays):
        assert lib.rt_trace_closest(dev._h, r.data_ptr(), n, d_hits.data_ptr(), None, None) == 0

    def hits(k):
        def f():
            assert lib.rt_trace_hits(dev._h, rays.data_ptr(), n, k, None, d_hits.data_ptr(), d_count.data_ptr(), None,
                                     None) == 0
        return f

    d = rays[:, 3:6]
    dn = d / torch.sqrt((d * d).sum(1, keepdim=True))
    slots_adv = torch.zeros((n, 8), dtype=torch.int32, device="cuda")

    def advance():   # rays with unit directions: t is the distance moved
        cur = rays.clone()
        cur[:, 3:6] = dn
        one = d_hits[:n]
        for j in range(8):
            closest(cur)
            t = one[:, 0]
            hit = torch.isfinite(t)
            slots_adv[:, j] = torch.where(hit, one.view(torch.int32)[:, 12], -1)
            step = torch.where(hit, t + PUSH, 0.0)
            cur[:, 0:3] += step[:, None] * dn
            cur[:, 6] = torch.where(hit, cur[:, 6] - step, 0.0)   # a finished ray is degenerate: never traversed

    # accuracy of the advancing method against the exact first-8 lists
    exact = dev.hits(rays, 8)
    advance()
    torch.cuda.synchronize()
    es, cnt = exact["slot"], exact["count"]
    valid = torch.arange(8, device="cuda")[None, :] < cnt[:, None]
    found = ((es[:, :, None] == slots_adv[:, None, :]) & valid[:, :, None]).any(2)
    lost = int((valid & ~found).sum())
    a_ok = slots_adv >= 0
    in_exact = ((slots_adv[:, :, None] == es[:, None, :]) & valid[:, None, :]).any(2)
    earlier = torch.tril(torch.ones((8, 8), dtype=torch.bool, device="cuda"), -1)[None]
    repeated = ((slots_adv[:, :, None] == slots_adv[:, None, :]) & earlier).any(2)
    extra = int((a_ok & (~in_exact | repeated)).sum())
    total = int(dev.all_hits(rays, 8)["offsets"][-1])

    cases = {"closest": closest, "hits_k1": hits(1), "hits_k2": hits(2), "hits_k4": hits(4), "hits_k8": hits(8),
             "all_hits_k8": lambda: dev.all_hits(rays, 8), "advance_k8": advance}
    runs = {k: [] for k in cases}
    for _ in range(ROUNDS):   # the cases interleaved, so a drift of the machine shows as spread, not as a difference
        for k, call in cases.items():
            runs[k].append(timed(call))
    ms = {k: statistics.median(v) for k, v in runs.items()}
    assert dev.status() == 0
    res = {"scene": name, "triangles": hs.triangle_count, "rays": n,
           "hits_first8": int(cnt.sum()), "hits_all": total, "rays_with_more_than_8": int((cnt == 8).sum()),
           "advance_push": PUSH, "advance_lost": lost, "advance_extra": extra,
           "ms": {k: round(v, 4) for k, v in ms.items()},
           "mrays_per_s": {k: round(n / ms[k] / 1e3, 1) for k in ms},
           "mrays_per_s_min_max": {k: [round(n / max(v) / 1e3, 1), round(n / min(v) / 1e3, 1)] for k, v in runs.items()}}
    dev.close()
    return res


out = {"reps": REPS, "rounds": ROUNDS, "lib": os.environ.get("RTAMD_HIP_LIB", "in-tree"),
       "scenes": [measure("office_proxy 1920x1080 camera rays, tile-major", *office()),
                  measure(f"random_tris {RANDOM_TRIS}, {RANDOM_RAYS} random rays", *random_scene())]}
print(json.dumps(out), flush=True)
