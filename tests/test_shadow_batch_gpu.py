"""All shadow rays of a bounce in one traversal phase (MI355X only).

A bounce's shadow rays go out as one batch of up to 32 lights.  Idle lanes of the wave take the
lights right after the owner's first; the owner traces the rest itself in later passes of the same
TRAVERSE phase and sets the same visibility bits helpers set.  Every case compares the fp64 image
within the suite's 1e-12 and the ray counts exactly against the CPU oracle, and the production
render bit for bit against the 4-wide diagnostic variant (RT_FLAG_WIDE_STATS).  The scenes
(tests/shadow_batch_scenes.py) are pinned on the CPU by tests/test_shadow_batch_scenes.py.
"""
import numpy as np
import pytest

import pyoracle
import rtamd
import shadow_batch_scenes as sbs

pytestmark = pytest.mark.gpu
TOL64 = 1e-12


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    return gpu_available


def counts(st):
    return [st.primary_rays, st.shadow_rays, st.reflection_rays]


def load(tmp_path, name, size=None):
    hs = rtamd.HostScene.load(sbs.write(tmp_path, name, size))
    hs.prepare()
    return hs, rtamd.DeviceScene(hs, 0)


def check(hs, dev, spp=1):
    """Production render against the oracle (image within 1e-12, counts exact) and against the
    diagnostic variant (bit for bit, counts exact); returns (image, Stats, diagnostic Stats)."""
    p = hs.render_params(0, 0, spp)
    p.out_format = rtamd.RT_OUT_RGB_F64
    img, st = dev.render(p)
    skipped = dev.debug_counters()["shadow_rays_skipped"]
    ref, cnt = pyoracle.Oracle(hs.raw, hs).render(p, pyoracle.MODE_REFERENCE)
    err = float(np.abs(img - ref).max())
    print(f"max |gpu - oracle| = {err:.3e}; rays {counts(st)}; not traced {skipped}")
    assert err <= TOL64
    assert counts(st) == [cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays]
    p.flags = rtamd.RT_FLAG_WIDE_STATS
    dimg, dst = dev.render(p)
    assert img.tobytes() == dimg.tobytes()
    assert counts(st) == counts(dst)
    assert skipped == dev.debug_counters()["shadow_rays_skipped"]
    return img, st, dst


@pytest.mark.parametrize("depth", [0, 3])
@pytest.mark.parametrize("n", sbs.LIGHT_COUNTS)
def test_light_counts(tmp_path, n, depth):
    # 1: baseline; 2, 3: one and two lights the owner traces after its first; 32: exactly one
    # batch; 33: the running light sum crosses a batch through the path state; 64: two batches
    hs, dev = load(tmp_path, f"lights{n}_depth{depth}")
    assert hs.render_params(0, 0, 1).n_lights == n
    img, st, dst = check(hs, dev)
    assert 2 * dst.closest_hits > 64 * 48
    assert st.shadow_rays == n * dst.closest_hits   # every hit is on a shadowable surface
    assert (st.reflection_rays > 0) == (depth > 0)


@pytest.mark.parametrize("size", [(8, 8), (24, 8), (64, 64)])
def test_helpers_and_owner_share_a_batch(tmp_path, size):
    # 8x8, 24x8: one and three waves with most lanes idle, helpers take lights; 64x64: full
    # waves, the owners trace all three lights themselves
    hs, dev = load(tmp_path, "lights3_depth3", size)
    check(hs, dev)


def test_sample_groups(tmp_path):
    hs, dev = load(tmp_path, "lights3_depth3", (24, 8))
    check(hs, dev, spp=2)


def test_tail_compaction_with_an_open_batch(tmp_path):
    # 72x40: 45 tiles over a whole persistent grid; the work heads run dry at once and the sparse
    # waves of the mirror's later bounces donate their lanes, shadow batches included
    hs, dev = load(tmp_path, "lights3_depth3", (72, 40))
    img, st, _ = check(hs, dev)
    # four frames in one launch: every frame the same image and a quarter of the rays
    import torch

    p = hs.render_params(0, 0, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    outs = [torch.zeros((40, 72, 3), dtype=torch.float64, device="cuda") for _ in range(4)]
    for flags in (0, rtamd.RT_FLAG_WIDE_STATS):
        p.flags = flags
        fst = dev.launch_frames(p, [o.data_ptr() for o in outs], stats=True)
        torch.cuda.synchronize()
        assert counts(fst) == [4 * c for c in counts(st)]
        for o in outs:
            assert o.cpu().numpy().tobytes() == img.tobytes()


def test_outer_iterations_do_not_grow_with_the_second_light(tmp_path):
    """The merge is in effect: on a floor that fills a 64x64 view every pixel hits and the 64 lanes
    of a wave (one 8x8 tile) stay in step, so a wave spends one iteration of its persistent loop on
    the closest-hit rays of a tile and one on its whole shadow batch, however many lights (<= 32)
    the batch has, plus one in which it finds the queue empty and leaves.  The diagnostic variant
    counts the iterations of all waves (outer_iters): 2 per tile + 1 per wave, the same with one
    light and with two.  (With one batch per light the two-light render took 3 per tile.)"""
    hs, dev = load(tmp_path, "floor_fill")
    check(hs, dev)
    p = hs.render_params(0, 0, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    p.flags = rtamd.RT_FLAG_WIDE_STATS
    assert p.n_lights == 2
    _, st2 = dev.render(p)
    it2 = dev.debug_counters()["outer_iters"]
    p.n_lights = 1
    _, st1 = dev.render(p)
    it1 = dev.debug_counters()["outer_iters"]
    print(f"outer_iters: {it2} with 2 lights, {it1} with 1 light")
    assert st2.closest_hits == st1.closest_hits == 64 * 64 == st1.shadow_rays
    assert st2.shadow_rays == 2 * 64 * 64
    assert it2 == it1
