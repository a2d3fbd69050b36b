"""Stack pushes and pops of the 4-wide node loop (MI355X only).

Every frame of tests/stack_fast_scenes.py (64x48, pinned on the CPU by
tests/test_stack_fast_scenes.py) on the three device trees, with the 8- and the 16-entry stack
ring, at 1 spp and at 4 spp (sample groups), against the CPU oracle within the suite's 1e-12 (fp64)
with exact ray counts; the 1 spp frame also bit for bit against the 4-wide diagnostic variant.  The
reference is the oracle's reference-semantics walk, for the deep scene its ordered walk (the
reference walk tests all 65536 triangles for every ray; the two agree:
test_stack_fast_scenes.py::test_oracle_modes_agree).

The diagnostic variant (8-entry ring) counts the wave-level node iterations whose capacity test
failed (slow push path) and those that popped while a lane had spilled entries (slow pop path),
rt_debug_counters words 40 and 41.
"""
import ctypes as C

import numpy as np
import pytest

import pyoracle
import rtamd
import stack_fast_scenes as sfs

pytestmark = pytest.mark.gpu
TOL64 = 1e-12
TREES = ["sbvh", "sah", "reference"]
SLOW_PUSH, SLOW_POP = 40, 41


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    return gpu_available


def counts(st):
    return [st.primary_rays, st.shadow_rays, st.reflection_rays]


class Ref:
    """A scene's host side and oracle frames, computed once and shared by the cases."""
    hosts = {}
    frames = {}

    @classmethod
    def host(cls, name, tmp_path_factory):
        if name not in cls.hosts:
            hs = rtamd.HostScene.load(sfs.write(name, tmp_path_factory.mktemp(name)))
            hs.prepare()
            cls.hosts[name] = (hs, pyoracle.Oracle(hs.raw, hs))
        return cls.hosts[name]

    @classmethod
    def frame(cls, name, spp, tmp_path_factory):
        if (name, spp) not in cls.frames:
            hs, orc = cls.host(name, tmp_path_factory)
            mode = pyoracle.MODE_ORDERED if name == "deep" else pyoracle.MODE_REFERENCE
            ref, cnt = orc.render(hs.render_params(0, 0, spp), mode)
            ref.setflags(write=False)
            cls.frames[(name, spp)] = (ref, cnt)
        return cls.frames[(name, spp)]


def raw_counters(dev):
    buf = (C.c_ulonglong * 42)()
    n = rtamd.hip_lib().rt_debug_counters(dev._h, buf, 42)
    assert n == 42, n
    return [int(x) for x in buf]


@pytest.mark.parametrize("ring", [8, 16])
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", sfs.NAMES)
def test_scene_matches_oracle(tmp_path_factory, name, tree, ring):
    hs, _ = Ref.host(name, tmp_path_factory)
    dev = rtamd.DeviceScene(hs, 0, tree=tree, stack_ring=ring)
    for spp in (1, 2):   # n: n x n samples per pixel
        ref, cnt = Ref.frame(name, spp, tmp_path_factory)
        p = hs.render_params(0, 0, spp)
        assert (p.camera.width, p.camera.height) == (sfs.W, sfs.H)
        p.out_format = rtamd.RT_OUT_RGB_F64
        img, st = dev.render(p)
        err = float(np.abs(img - ref).max())
        print(f"{name} {tree} ring {ring} spp {spp * spp}: max |gpu - oracle| = {err:.3e}; rays {counts(st)}")
        assert err <= TOL64
        assert counts(st) == counts(cnt)
        if spp == 1:
            p.flags = rtamd.RT_FLAG_WIDE_STATS
            dimg, dst = dev.render(p)
            assert img.tobytes() == dimg.tobytes()
            assert counts(dst) == counts(cnt)


def diag(tmp_path_factory, name, tree="sbvh"):
    hs, _ = Ref.host(name, tmp_path_factory)
    _, cnt = Ref.frame(name, 1, tmp_path_factory)
    dev = rtamd.DeviceScene(hs, 0, tree=tree)
    p = hs.render_params(0, 0, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    p.flags = rtamd.RT_FLAG_WIDE_STATS
    _, st = dev.render(p)
    words = raw_counters(dev)
    named = dev.debug_counters()
    print(f"{name} {tree}: node iterations {named['node_iters']}, slow push {words[SLOW_PUSH]}, slow pop {words[SLOW_POP]}, "
          f"stack spills {named['stack_spills']}")
    return st, cnt, named, words


@pytest.mark.parametrize("tree", TREES)
def test_deep_scene_takes_both_paths_in_one_frame(tmp_path_factory, tree):
    _, _, named, words = diag(tmp_path_factory, "deep", tree)
    assert named["stack_spills"] > 0
    assert words[SLOW_PUSH] > 0 and words[SLOW_POP] > 0
    assert named["node_iters"] - words[SLOW_PUSH] > 0
    assert named["node_iters"] - words[SLOW_POP] > 0


@pytest.mark.parametrize("tree", TREES)
def test_flat_scene_never_leaves_the_fast_paths(tmp_path_factory, tree):
    _, _, named, words = diag(tmp_path_factory, "flat", tree)
    assert named["node_iters"] > 0
    assert named["stack_spills"] == 0 and words[SLOW_PUSH] == 0 and words[SLOW_POP] == 0


@pytest.mark.parametrize("name", sfs.NAMES)
def test_traversal_counters_match_oracle_replica(tmp_path_factory, name):
    # as tests/test_gpu_parity.py pins them: the canonical diagnostic variant's node visits, triangle
    # tests and closest hits equal the oracle's ordered replica; the 4-wide diagnostic variant walks
    # the device hierarchy, not the oracle's, and shares the closest hits
    hs, orc = Ref.host(name, tmp_path_factory)
    p = hs.render_params(0, 0, 1)
    _, cnt = orc.render(p, pyoracle.MODE_ORDERED)
    dev = rtamd.DeviceScene(hs, 0, tree="reference")
    p.flags = rtamd.RT_FLAG_TRAVERSAL_STATS
    _, st = dev.render(p)
    assert (st.node_visits, st.tri_tests, st.closest_hits) == (cnt.node_visits, cnt.tri_tests, cnt.closest_hits)
    p.flags = rtamd.RT_FLAG_WIDE_STATS
    _, wst = dev.render(p)
    assert wst.closest_hits == cnt.closest_hits
