"""Vertex-update rates (dev tool, needs the MI355X): rt_scene_update_vertices against the only
alternative the parent commit has, a fresh rt_scene_upload_ex of the moved scene, on the office proxy
and the cornell room, each with the default device tree (RT_TREE_SBVH) and with RT_TREE_SAH.

The motion is tests/update_cases.py's for generated scenes: the vertices of odd mesh ids translated by
f x the vertex box's diagonal x a unit vector per mesh (numpy default_rng(0)), at three sizes f.  For
each scene and size the host scene is moved (rt_host_update_vertices, timed on the host clock), then:
  update_ms    rt_scene_update_vertices, from HIP events around the call on the null stream, REPS
               calls alternating between the moved and the original positions so that every call
               changes every moved record (copies of the three arrays, records kernel, one refit
               kernel per height); median and [min, max] over 5 rounds;
  upload_ms    rt_scene_upload_seconds of a fresh upload of the same moved scene: build_s + copy_s;
  mrays_s      primary + shadow + reflection rays of a 1920 x 1080 frame over the median
               rt_last_kernel_ms of REPS frames, on the updated scene (refitted boxes of the original
               topology) beside the same frame on the fresh upload (a hierarchy built for the moved
               geometry), the two interleaved.
Before anything is timed the updated scene's frame is checked to equal the fresh upload's bit for
bit.  No figure carries a pass threshold.  RTAMD_HIP_LIB selects the library.

usage: python tools/update_rate.py [REPS]
"""
import json
import os
import statistics
import sys
import time
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
TREES = ("sbvh", "sah")   # the default device tree (spatial splits: clipped leaf boxes) and object splits only


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


def frame_rate(dev, p, out):
    """(rays of the frame, median kernel ms of REPS frames)."""
    st = dev.launch(p, out.data_ptr(), stats=True)
    rays = st.primary_rays + st.shadow_rays + st.reflection_rays
    ms = []
    for _ in range(WARM + REPS):
        dev.launch(p, out.data_ptr())
        ms.append(dev.last_kernel_ms())
    return rays, statistics.median(ms[WARM:])


def update_ms(dev, states):
    """ms per rt_scene_update_vertices call, the calls alternating between two states."""
    rounds = []
    for _ in range(ROUNDS):
        for i in range(WARM):
            dev.update_vertices(*states[i % 2])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(REPS):
            dev.update_vertices(*states[(WARM + i) % 2])
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / REPS)
    return rounds


results = []
for name, tree in [(n, t) for n in SCENES for t in TREES]:
    hs = rtamd.HostScene.generate(name)
    hs.prepare()
    p = hs.render_params(W, H, 1)
    out_u = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    out_f = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    dev = rtamd.DeviceScene(hs, 0, tree=tree)
    b_upload = dev.device_bytes
    state_a = host_arrays(hs)
    rays0, ms0 = frame_rate(dev, p, out_u)
    row = {"scene": name, "tree": tree, "triangles": hs.triangle_count, "vertices": int(hs.soa.contents.n_vertices),
           "upload_ms_original": round(1e3 * sum(dev.upload_seconds), 3),
           "mrays_s_original": round(rays0 / ms0 / 1e3, 1), "device_bytes_upload": b_upload, "moves": []}
    for f in FACTORS:
        hs.update_vertices(state_a[0])   # moved from the original positions, not cumulatively
        P = moved_positions(hs, f)
        t0 = time.perf_counter()
        hs.update_vertices(P)
        host_ms = 1e3 * (time.perf_counter() - t0)
        state_b = host_arrays(hs)
        dev.update(hs)
        fresh = rtamd.DeviceScene(hs, 0, tree=tree)
        dev.launch(p, out_u.data_ptr())
        fresh.launch(p, out_f.data_ptr())
        torch.cuda.synchronize()
        assert bool((out_u.view(torch.int32) == out_f.view(torch.int32)).all()), "updated frame differs from fresh upload"
        ru, rf, mu, mf = 0, 0, [], []
        for _ in range(ROUNDS):   # interleaved: a drift of the machine shows as spread
            ru, m = frame_rate(dev, p, out_u)
            mu.append(m)
            rf, m = frame_rate(fresh, p, out_f)
            mf.append(m)
        assert ru == rf
        up = update_ms(dev, (state_b, state_a))
        dev.update_vertices(*state_b)
        b, c = fresh.upload_seconds
        row["moves"].append({
            "factor": f, "host_update_ms": round(host_ms, 3),
            "update_ms": round(statistics.median(up), 4), "update_ms_min_max": [round(min(up), 4), round(max(up), 4)],
            "upload_ms": round(1e3 * (b + c), 3), "upload_build_ms": round(1e3 * b, 3), "upload_copy_ms": round(1e3 * c, 3),
            "rays": int(ru),
            "mrays_s_updated": round(ru / statistics.median(mu) / 1e3, 1),
            "mrays_s_fresh": round(rf / statistics.median(mf) / 1e3, 1),
            "frame_ms_updated": round(statistics.median(mu), 4), "frame_ms_fresh": round(statistics.median(mf), 4),
            "frame_ms_updated_min_max": [round(min(mu), 4), round(max(mu), 4)],
            "frame_ms_fresh_min_max": [round(min(mf), 4), round(max(mf), 4)]})
        fresh.close()
    row["device_bytes_after_update"] = dev.device_bytes
    assert dev.status() == 0
    dev.close()
    results.append(row)
print(json.dumps({"frame": f"{W}x{H}", "reps": REPS, "rounds": ROUNDS, "lib": os.environ.get("RTAMD_HIP_LIB", "in-tree"),
                  "scenes": results}), flush=True)
