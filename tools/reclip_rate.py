"""Re-clipping update rates (dev tool, needs the MI355X): rt_scene_update_vertices_ex with
RT_UPDATE_RECLIP beside the plain refit and a fresh upload, on the office proxy and the cornell room
with the default device tree (RT_TREE_SBVH), and the refitted RT_TREE_SAH tree for comparison
(DESIGN.md §25).  The method is tools/update_rate.py's.

The motion: the vertices of odd mesh ids translated by f x the vertex box's diagonal x a unit vector
per mesh (numpy default_rng(0)), at three sizes f, always from the original positions.  Per scene
and size three scenes of the same sbvh upload are compared -- one plainly refitted, one re-clipped,
one freshly uploaded from the moved scene -- and one sah upload, plainly refitted:
  update_ms    HIP events around REPS calls on the null stream alternating between the moved and the
               original positions; median and [min, max] over 5 rounds; plain and re-clipping;
  frame_ms     median rt_last_kernel_ms of REPS 1920 x 1080 frames, 5 rounds, the four scenes interleaved.
Before anything is timed the three sbvh frames are checked to be equal bit for bit.  No figure
carries a pass threshold.  RTAMD_HIP_LIB selects the library.

usage: python tools/reclip_rate.py [REPS]
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

REPS = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 20
ROUNDS = 5
WARM = 3
W, H = 1920, 1080
FACTORS = (0.01, 0.1, 0.3)
SCENES = ("office", "cornell")


def moved_positions(hs, factor):
    soa = hs.soa_arrays()
    P, mid = soa["vertex_pos"].copy(), soa["vertex_mesh_id"]
    e = P.max(axis=0) - P.min(axis=0)
    diag = float(np.sqrt((e * e).sum()))
    rng = np.random.default_rng(0)
    for m in range(1, int(mid.max()) + 1, 2):
        u = rng.normal(size=3)
        P[mid == m] += factor * diag * (u / np.sqrt((u * u).sum()))
    return P


def host_arrays(hs):
    return tuple(hs.soa_arrays()[k].copy() for k in ("vertex_pos", "vertex_normals", "face_normals"))


def frame_ms(dev, p, out):
    ms = []
    for _ in range(WARM + REPS):
        dev.launch(p, out.data_ptr())
        ms.append(dev.last_kernel_ms())
    return statistics.median(ms[WARM:])


def update_ms(dev, states, reclip):
    rounds = []
    for _ in range(ROUNDS):
        for i in range(WARM):
            dev.update_vertices(*states[i % 2], reclip=reclip)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(REPS):
            dev.update_vertices(*states[(WARM + i) % 2], reclip=reclip)
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / REPS)
    return rounds


def med(xs):
    return round(statistics.median(xs), 4)


results = []
for name in SCENES:
    hs = rtamd.HostScene.generate(name)
    hs.prepare()
    p = hs.render_params(W, H, 1)
    outs = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(4)]
    plain, tight, sah = rtamd.DeviceScene(hs, 0), rtamd.DeviceScene(hs, 0), rtamd.DeviceScene(hs, 0, tree="sah")
    b_upload = tight.device_bytes
    state_a = host_arrays(hs)
    clip, _ = rtamd.clip_regions(hs)
    row = {"scene": name, "triangles": hs.triangle_count, "records": len(clip),
           "cut_records": int(np.isfinite(clip).any(axis=1).sum()), "frame_ms_original": round(frame_ms(tight, p, outs[1]), 4),
           "moves": []}
    for f in FACTORS:
        hs.update_vertices(state_a[0])   # moved from the original positions, not cumulatively
        hs.update_vertices(moved_positions(hs, f))
        state_b = host_arrays(hs)
        plain.update(hs)
        tight.update(hs, reclip=True)
        sah.update(hs)
        fresh = rtamd.DeviceScene(hs, 0)
        scenes = (plain, tight, fresh, sah)
        for d, o in zip(scenes, outs):
            d.launch(p, o.data_ptr())
        torch.cuda.synchronize()
        for o in outs[1:3]:
            assert bool((o.view(torch.int32) == outs[0].view(torch.int32)).all()), "frames differ"
        ms = [[] for _ in scenes]
        for _ in range(ROUNDS):   # interleaved: a drift of the machine shows as spread
            for k, (d, o) in enumerate(zip(scenes, outs)):
                ms[k].append(frame_ms(d, p, o))
        up_plain = update_ms(plain, (state_b, state_a), False)
        up_tight = update_ms(tight, (state_b, state_a), True)
        row["moves"].append({
            "factor": f,
            "update_ms_plain": med(up_plain), "update_ms_plain_min_max": [round(min(up_plain), 4), round(max(up_plain), 4)],
            "update_ms_reclip": med(up_tight), "update_ms_reclip_min_max": [round(min(up_tight), 4), round(max(up_tight), 4)],
            "frame_ms_plain": med(ms[0]), "frame_ms_reclip": med(ms[1]), "frame_ms_fresh": med(ms[2]),
            "frame_ms_sah_refit": med(ms[3]),
            "frame_ms_min_max": {k: [round(min(m), 4), round(max(m), 4)]
                                 for k, m in zip(("plain", "reclip", "fresh", "sah_refit"), ms)}})
        fresh.close()
    row["device_bytes_upload"] = b_upload
    row["device_bytes_after_plain"] = plain.device_bytes
    row["device_bytes_after_reclip"] = tight.device_bytes
    for d in (plain, tight, sah):
        assert d.status() == 0
        d.close()
    results.append(row)
print(json.dumps({"frame": f"{W}x{H}", "reps": REPS, "rounds": ROUNDS, "lib": os.environ.get("RTAMD_HIP_LIB", "in-tree"),
                  "scenes": results}), flush=True)
