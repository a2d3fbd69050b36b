"""The optimised device hierarchy on the GPU (rt_upload_options.tree_opt; MI355X only).

Pixels and ray counts cannot depend on the hierarchy (the closest hit is the smallest
(t, slot) over a conservative superset).  Every scene is rendered with tree_opt = -1 (the builder's
tree), 1 (one pass) and the default (by size: on) -- the deep tunnel, which spills, on both stack
rings: the fp64 frames must be bit-identical to each other with equal ray counts, and within the
suite's 1e-12 of the CPU oracle with exact counts.  The query kernels share the image: one
closest-hit / occlusion case runs on the optimised office.  On the office the 4-wide diagnostic
variant's node visits plus triangle tests of closest-hit rays (no lights) must not exceed those of
the builder's tree.
"""
import numpy as np
import pytest

import pyoracle
import query_cases as qc
import rtamd
import tree_opt_scenes as tos

pytestmark = pytest.mark.gpu
TOL64 = 1e-12
# scene: (width, height, n x n samples); 0 x 0 = the scene file's 64 x 48
FRAMES = {"deep": (0, 0, 1), "flat": (0, 0, 1), "occluder": (0, 0, 1), "fan": (0, 0, 1), "split_stress": (0, 0, 1),
          "cornell": (97, 61, 2), "random20k": (64, 48, 1), "office": (160, 90, 1)}
MODES = [-1, 1, 0]


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    return gpu_available


def counts(st):
    return [st.primary_rays, st.shadow_rays, st.reflection_rays]


@pytest.mark.parametrize("name", list(FRAMES))
def test_frames_do_not_depend_on_tree_opt(tmp_path_factory, name):
    hs = tos.host(name, tmp_path_factory)
    w, h, spp = FRAMES[name]
    p = hs.render_params(w, h, spp)
    # the deep scene's reference walk tests every triangle for every ray; its ordered walk agrees
    # (tests/test_stack_fast_scenes.py::test_oracle_modes_agree)
    mode = pyoracle.MODE_ORDERED if name == "deep" else pyoracle.MODE_REFERENCE
    ref, cnt = pyoracle.Oracle(hs.raw, hs).render(p, mode)
    p.out_format = rtamd.RT_OUT_RGB_F64
    first = None
    for ring in ((8, 16) if name == "deep" else (0,)):
        for t in MODES:
            dev = rtamd.DeviceScene(hs, 0, tree_opt=t, stack_ring=ring)
            img, st = dev.render(p)
            dev.close()
            if first is None:
                first = img
                err = float(np.abs(img - ref).max())
                print(f"{name}: max |gpu - oracle| = {err:.3e}; rays {counts(st)}")
                assert err <= TOL64
            assert img.tobytes() == first.tobytes(), (name, ring, t)
            assert counts(st) == counts(cnt), (name, ring, t)


def test_queries_on_the_optimised_office():
    hs, orc, P, vidx, perm = qc.scene("office")
    rays = qc.random_rays(hs)
    want = qc.expected(("office", "random"), orc, rays, pyoracle.MODE_REFERENCE)
    dev = rtamd.DeviceScene(hs, 0)   # default: optimised
    got, st = dev.trace(rays, stats=True)
    qc.check_hits(got, want, rays, P, vidx, perm)
    assert st.rays == len(rays) and st.hits == int(want["hit"].sum()) and st.watchdog == 0
    occ = dev.trace(rays, occluded=True)
    assert np.array_equal(occ.astype(bool), want["hit"])


def test_office_traversal_work_does_not_rise(tmp_path_factory):
    hs = tos.host("office", tmp_path_factory)
    p = hs.render_params(160, 90, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    p.flags = rtamd.RT_FLAG_WIDE_STATS
    p.n_lights = 0   # closest-hit rays only: the counts do not depend on any-hit early exits
    work = {}
    for t in (-1, 0):
        dev = rtamd.DeviceScene(hs, 0, tree_opt=t)
        _, st = dev.render(p)
        dev.close()
        work[t] = (st.node_visits, st.tri_tests)
    print(f"office 160x90, closest-hit rays: node visits + triangle tests {sum(work[-1])} {work[-1]} with tree_opt=-1, "
          f"{sum(work[0])} {work[0]} with the default")
    assert sum(work[0]) <= sum(work[-1])
