"""Time per changed state of a moving scene (dev tool, needs the MI355X): rt_scene_update_positions
against the path the parent commit has, on the office proxy and the cornell room, each with the
default device tree re-clipped (RT_TREE_SBVH + RT_UPDATE_RECLIP) and with RT_TREE_SAH.

The motion is tests/update_cases.py's for generated scenes at 0.1 of the vertex box's diagonal; every
call alternates between the moved and the original positions, so each changes every moved record.
Three paths, in one run:
  a  rt_host_update_vertices (normals on the host, one thread; wall clock per call) plus
     rt_scene_update_vertices_ex with its three arrays (HIP events around REPS calls on the null
     stream): host_ms + device_ms = a_ms.  Also the pair timed together by the wall clock, a
     synchronisation at the end of the REPS pairs: a_wall_ms;
  b  rt_scene_update_positions from a host array: HIP events around REPS calls (b_event_ms) and the
     wall clock around the same calls with a synchronisation at the end (b_wall_ms, which holds the
     call's host loops over the positions);
  c  rt_scene_update_positions from a device tensor: the wall clock around REPS calls, each with its
     one synchronisation, and a synchronisation at the end (c_wall_ms).
Each figure is the median of 5 rounds of REPS calls after 3 warm-up calls, with [min, max].  Before
anything is timed the normal records after b and c are checked to equal those after a byte for byte.
No figure carries a pass threshold.  RTAMD_HIP_LIB selects the library.

usage: python tools/positions_rate.py [REPS]
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
FACTOR = 0.1
SCENES = ("office", "cornell")
MODES = (("sbvh", True), ("sah", False))   # (device tree, RT_UPDATE_RECLIP)


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


def rounds_of(call, events=False):
    """ms per call over ROUNDS rounds of REPS calls; call(i) issues call i.  events: HIP events on
    the null stream instead of the wall clock (which ends with a synchronisation)."""
    out = []
    for _ in range(ROUNDS):
        for i in range(WARM):
            call(i)
        torch.cuda.synchronize()
        if events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(REPS):
                call(WARM + i)
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / REPS)
        else:
            t0 = time.perf_counter()
            for i in range(REPS):
                call(WARM + i)
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0) / REPS)
    return out


def figure(rounds):
    return {"median": round(statistics.median(rounds), 4), "min_max": [round(min(rounds), 4), round(max(rounds), 4)]}


results = []
for name, (tree, reclip) in [(n, m) for n in SCENES for m in MODES]:
    hs = rtamd.HostScene.generate(name)
    hs.prepare()
    pos = [hs.soa_arrays()["vertex_pos"].copy(), moved_positions(hs, FACTOR)]
    dev_t = [torch.from_numpy(p).cuda() for p in pos]
    arrays = []
    for p in pos:
        hs.update_vertices(p)
        arrays.append(tuple(hs.soa_arrays()[k].copy() for k in ("vertex_pos", "vertex_normals", "face_normals")))
    dev_a = rtamd.DeviceScene(hs, 0, tree=tree)
    dev_b = rtamd.DeviceScene(hs, 0, tree=tree)
    dev_b.set_triangle_order(hs.slot_triangles())

    # the three paths give the same records
    dev_a.update_vertices(*arrays[1], reclip=reclip)
    want = {k: dev_a.debug_scene_image(k) for k in ("nodes4", "tris", "tnorm")}
    for src in (pos[1], dev_t[1]):
        dev_b.update_positions(pos[0], reclip=reclip)
        dev_b.update_positions(src, reclip=reclip)
        for k, w in want.items():
            assert np.array_equal(dev_b.debug_scene_image(k).view(np.uint32), w.view(np.uint32)), (name, tree, k)

    host = rounds_of(lambda i: hs.update_vertices(pos[i % 2]))
    a_dev = rounds_of(lambda i: dev_a.update_vertices(*arrays[i % 2], reclip=reclip), events=True)

    def pair(i):
        hs.update_vertices(pos[i % 2])
        dev_a.update(hs, reclip=reclip)

    a_wall = rounds_of(pair)
    b_event = rounds_of(lambda i: dev_b.update_positions(pos[i % 2], reclip=reclip), events=True)
    b_wall = rounds_of(lambda i: dev_b.update_positions(pos[i % 2], reclip=reclip))
    c_wall = rounds_of(lambda i: dev_b.update_positions(dev_t[i % 2], reclip=reclip))
    assert dev_a.status() == 0 and dev_b.status() == 0
    results.append({"scene": name, "tree": tree, "reclip": reclip, "triangles": hs.triangle_count,
                    "vertices": int(hs.soa.contents.n_vertices),
                    "a_host_ms": figure(host), "a_device_ms": figure(a_dev),
                    "a_ms": round(statistics.median(host) + statistics.median(a_dev), 4), "a_wall_ms": figure(a_wall),
                    "b_event_ms": figure(b_event), "b_wall_ms": figure(b_wall), "c_wall_ms": figure(c_wall),
                    "device_bytes_a": dev_a.device_bytes, "device_bytes_b": dev_b.device_bytes})
    dev_a.close()
    dev_b.close()
print(json.dumps({"factor": FACTOR, "reps": REPS, "rounds": ROUNDS, "warm": WARM,
                  "lib": os.environ.get("RTAMD_HIP_LIB", "in-tree"), "scenes": results}), flush=True)
