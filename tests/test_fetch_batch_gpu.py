"""One batch of loads per triangle and material record (MI355X only).

The leaf loop issues all five loads of a triangle record ahead of its first branch, and SHADE
fetches what a branch needs of a material, and the normal record, in one or two round trips.  Only
the point where loads are issued moved, so every frame here (64x48, tests/fetch_batch_scenes.py,
pinned on the CPU by tests/test_fetch_batch_scenes.py) is compared with the CPU oracle within the
suite's 1e-12 (fp64) with exact ray counts, on the three device trees, and the production render
bit for bit against the 4-wide diagnostic variant.
"""
import numpy as np
import pytest

import fetch_batch_scenes as fbs
import pyoracle
import rtamd

pytestmark = pytest.mark.gpu
TOL64 = 1e-12
TREES = ["sbvh", "sah", "reference"]


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    return gpu_available


def counts(st):
    return [st.primary_rays, st.shadow_rays, st.reflection_rays]


class Ref:
    """A scene's host side and oracle frame, computed once and shared by the trees."""
    cache = {}

    @classmethod
    def get(cls, name, tmp_path_factory, spp=1):
        if (name, spp) not in cls.cache:
            write = fbs.write_leaf if name == "leaf" else fbs.write_material
            hs = rtamd.HostScene.load(write(tmp_path_factory.mktemp(name)))
            hs.prepare()
            p = hs.render_params(0, 0, spp)
            ref, cnt = pyoracle.Oracle(hs.raw, hs).render(p, pyoracle.MODE_REFERENCE)
            ref.setflags(write=False)
            cls.cache[(name, spp)] = (hs, ref, [cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays])
        return cls.cache[(name, spp)]


def check(hs, dev, ref, ref_counts, spp=1):
    p = hs.render_params(0, 0, spp)
    assert (p.camera.width, p.camera.height) == (fbs.W, fbs.H)
    p.out_format = rtamd.RT_OUT_RGB_F64
    img, st = dev.render(p)
    err = float(np.abs(img - ref).max())
    print(f"max |gpu - oracle| = {err:.3e}; rays {counts(st)}")
    assert err <= TOL64
    assert counts(st) == ref_counts
    p.flags = rtamd.RT_FLAG_WIDE_STATS
    dimg, dst = dev.render(p)
    assert img.tobytes() == dimg.tobytes()
    assert counts(dst) == ref_counts
    return st, dst


@pytest.mark.parametrize("tree", TREES)
def test_leaf_scene(tmp_path_factory, tree):
    hs, ref, rc = Ref.get("leaf", tmp_path_factory)
    st, dst = check(hs, rtamd.DeviceScene(hs, 0, tree=tree), ref, rc)
    assert st.shadow_rays > 0 and st.reflection_rays > 0
    assert 0 < dst.closest_hits


@pytest.mark.parametrize("ring", [8, 16])
def test_leaf_scene_on_both_stack_rings(tmp_path_factory, ring):
    hs, ref, rc = Ref.get("leaf", tmp_path_factory)
    check(hs, rtamd.DeviceScene(hs, 0, stack_ring=ring), ref, rc)


@pytest.mark.parametrize("tree", TREES)
def test_material_scene(tmp_path_factory, tree):
    hs, ref, rc = Ref.get("material", tmp_path_factory)
    assert hs.render_params(0, 0, 1).n_lights == 2 and hs.render_params(0, 0, 1).max_depth == 3
    st, _ = check(hs, rtamd.DeviceScene(hs, 0, analytic=True, tree=tree), ref, rc)
    assert st.shadow_rays > 0 and st.reflection_rays > 0


@pytest.mark.parametrize("name", ["leaf", "material"])
def test_sample_groups(tmp_path_factory, name):
    # spp > 1 runs the sample-group variants, which keep reading materials field by field
    hs, ref, rc = Ref.get(name, tmp_path_factory, spp=2)
    check(hs, rtamd.DeviceScene(hs, 0, analytic=(name == "material")), ref, rc, spp=2)
