"""Zero-term shadow rays on the GPU (MI355X only).

A shadow ray whose light does not face the surface (max(0, n.l) == 0) of a material with
shininess > 0 and finite coefficients, all light colours finite, adds exactly +-0 to the light sum
whatever it finds: the production kernels count it and do not trace it.  Every case here compares
the fp64 image within the suite's 1e-12 and the ray counts exactly against the CPU oracle, and bit
for bit against the same launch rendered by the 4-wide diagnostic variant (RT_FLAG_WIDE_STATS),
which traces every ray and only counts the marked ones (debug counter shadow_rays_skipped).
"""
import numpy as np
import pytest

import pyoracle
import rtamd
import zero_term_scenes as zts

pytestmark = pytest.mark.gpu
TOL64 = 1e-12


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    return gpu_available


def counts(st):
    return [st.primary_rays, st.shadow_rays, st.reflection_rays]


def load(tmp_path, name, size=None, edit=None, **upload):
    hs = rtamd.HostScene.load(zts.write(tmp_path, name, size))
    hs.prepare()
    if edit is not None:
        edit(hs)
    return hs, rtamd.DeviceScene(hs, 0, **upload)


def render_both(hs, dev, spp=1, edit_params=None):
    """Production and diagnostic render of one launch: (image, Stats, skipped, diagnostic Stats)."""
    p = hs.render_params(0, 0, spp)
    p.out_format = rtamd.RT_OUT_RGB_F64
    if edit_params is not None:
        edit_params(p)
    img, st = dev.render(p)
    skipped = dev.debug_counters()["shadow_rays_skipped"]
    p.flags = rtamd.RT_FLAG_WIDE_STATS
    dimg, dst = dev.render(p)
    marked = dev.debug_counters()["shadow_rays_skipped"]
    assert img.tobytes() == dimg.tobytes()   # bit for bit, NaNs included
    assert counts(st) == counts(dst)
    assert skipped == marked   # the diagnostic variant marks the rays the production one skips
    return img, st, skipped, dst


def check(hs, dev, spp=1):
    """render_both + the oracle's reference mode: fp64 image within 1e-12, ray counts exact."""
    img, st, skipped, dst = render_both(hs, dev, spp)
    p = hs.render_params(0, 0, spp)
    ref, cnt = pyoracle.Oracle(hs.raw, hs).render(p, pyoracle.MODE_REFERENCE)
    assert np.abs(img - ref).max() <= TOL64
    assert counts(st) == [cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays]
    return img, st, skipped, dst


def test_floor_with_two_lights(tmp_path):
    hs, dev = load(tmp_path, "floor_two_lights")
    img, st, skipped, dst = check(hs, dev)
    hits = dst.closest_hits
    assert 0 < hits < st.primary_rays
    assert st.shadow_rays == 2 * hits
    assert skipped == hits   # the light 50 below the floor, at every hit; never the one above


def test_shininess_zero_skips_nothing(tmp_path):
    hs, dev = load(tmp_path, "floor_shininess_zero")
    img, st, skipped, dst = check(hs, dev)
    assert skipped == 0
    assert st.shadow_rays == 2 * dst.closest_hits
    hs2, dev2 = load(tmp_path, "floor_two_lights")
    img2, _, _, _ = render_both(hs2, dev2)
    assert np.abs(img - img2).max() > 0.05   # pow(0, 0) = 1: the light below adds ks


def test_non_finite_light_colour_skips_nothing(tmp_path):
    hs, dev = load(tmp_path, "floor_two_lights")

    def edit(p):
        p.lights[1].color[0] = float("inf")   # the light below the floor: inf * 0 = NaN

    img, st, skipped, _ = render_both(hs, dev, edit_params=edit)
    assert skipped == 0
    assert np.isnan(img[..., 0]).any() and not np.isnan(img[..., 1:]).any()
    # finite again: the same scene skips again (the flag is the launch's, not the scene's)
    _, _, skipped2, dst = render_both(hs, dev)
    assert skipped2 == dst.closest_hits


def test_non_finite_specular_skips_nothing(tmp_path):
    def edit(hs):
        hs.soa.contents.mat_specular[1] = float("inf")   # ks.g of the floor: inf * pow(0, 20) = NaN

    hs, dev = load(tmp_path, "floor_two_lights", edit=edit)
    img, st, skipped, _ = render_both(hs, dev)
    assert skipped == 0
    assert np.isnan(img[..., 1]).any() and not np.isnan(img[..., 0]).any()


def test_lights_in_and_next_to_the_surface_plane(tmp_path):
    hs, dev = load(tmp_path, "grazing")
    img, st, skipped, dst = check(hs, dev)
    hits = dst.closest_hits
    assert st.shadow_rays == 4 * hits
    # the light 1e-9 below the plane at every hit, the one 1e-9 above at none, the one above never;
    # the light in the plane wherever the hit point's rounded height makes n.l <= 0
    assert hits <= skipped <= 2 * hits


def test_phong_normals_terminator(tmp_path):
    hs, dev = load(tmp_path, "phong_terminator")
    img, st, skipped, _ = check(hs, dev)
    assert 0 < skipped < st.shadow_rays


def test_owner_first_light_skipped_reflection_still_traced(tmp_path):
    hs, dev = load(tmp_path, "mirror_lights_behind")
    img, st, skipped, _ = check(hs, dev)
    assert st.reflection_rays > 0
    assert skipped > 0
    hs2, dev2 = load(tmp_path, "floor_below_first")
    _, st2, skipped2, dst2 = check(hs2, dev2)
    assert skipped2 == dst2.closest_hits


def test_forty_lights_cross_the_batch(tmp_path):
    hs, dev = load(tmp_path, "many_lights")
    img, st, skipped, _ = check(hs, dev)
    assert hs.render_params(0, 0, 1).n_lights == 40
    assert 0 < skipped < st.shadow_rays


def test_one_light_only(tmp_path):
    hs, dev = load(tmp_path, "one_light")
    img, st, skipped, dst = check(hs, dev)
    assert st.shadow_rays == dst.closest_hits
    assert 0 < skipped < st.shadow_rays


def test_textured_material():
    hs = rtamd.HostScene.generate("cornell")   # FLAT, PHONG, a textured poster, a mirror
    hs.prepare()
    dev = rtamd.DeviceScene(hs, 0)
    p = hs.render_params(40, 30, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    img, st = dev.render(p)
    skipped = dev.debug_counters()["shadow_rays_skipped"]
    ref, cnt = pyoracle.Oracle(hs.raw, hs).render(p, pyoracle.MODE_REFERENCE)
    assert np.abs(img - ref).max() <= TOL64
    assert counts(st) == [cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays]
    p.flags = rtamd.RT_FLAG_WIDE_STATS
    dimg, dst = dev.render(p)
    assert img.tobytes() == dimg.tobytes() and counts(st) == counts(dst)
    assert 0 < skipped == dev.debug_counters()["shadow_rays_skipped"]


@pytest.mark.parametrize("spp", [2, 3])   # 4 samples: sample groups; 9: one lane per pixel
@pytest.mark.parametrize("name", ["many_lights", "phong_terminator"])
def test_supersampled(tmp_path, name, spp):
    hs, dev = load(tmp_path, name, size=(12, 9))
    img, st, skipped, _ = check(hs, dev, spp)
    assert 0 < skipped < st.shadow_rays


def test_adaptive_pass(tmp_path):
    import torch

    hs, dev = load(tmp_path, "phong_terminator")
    orc = pyoracle.Oracle(hs.raw, hs)
    p = hs.render_params(0, 0, 1)
    h, w = p.camera.height, p.camera.width
    prim, _ = orc.render(p)
    ref, cnt, sel = orc.adaptive(p, prim, subp=4, threshold=0.02)
    assert sel.sum() > 0
    d_prim = torch.from_numpy(prim).cuda()
    p.out_format = rtamd.RT_OUT_RGB_F64
    out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    st, nsel = dev.launch_adaptive(p, d_prim.data_ptr(), out.data_ptr(), 4, 0.02, stats=True)
    skipped = dev.debug_counters()["shadow_rays_skipped"]
    assert nsel == int(sel.sum())
    assert np.abs(out.cpu().numpy() - ref).max() <= TOL64
    assert counts(st) == [cnt.primary_rays, cnt.shadow_rays, cnt.reflection_rays]
    assert 0 < skipped < st.shadow_rays
    p.flags = rtamd.RT_FLAG_WIDE_STATS
    dout = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    dst, _ = dev.launch_adaptive(p, d_prim.data_ptr(), dout.data_ptr(), 4, 0.02, stats=True)
    assert out.cpu().numpy().tobytes() == dout.cpu().numpy().tobytes()
    assert counts(st) == counts(dst)
    assert skipped == dev.debug_counters()["shadow_rays_skipped"]


@pytest.mark.parametrize("tree", ["sbvh", "sah", "reference"])
@pytest.mark.parametrize("ring", [8, 16])
def test_device_trees_and_ring_depths(tmp_path, tree, ring):
    hs, dev = load(tmp_path, "many_lights", tree=tree, stack_ring=ring)
    img, st, skipped, _ = check(hs, dev)
    assert 0 < skipped < st.shadow_rays


def test_tail_compaction(tmp_path):
    # 24x16: six tiles over a whole persistent grid, the work heads run dry at once and sparse
    # waves donate their lanes (shadow batches in flight included) to others of their block
    hs, dev = load(tmp_path, "mirror_lights_behind", size=(24, 16))
    img, st, skipped, _ = check(hs, dev)
    assert skipped > 0
    hs2, dev2 = load(tmp_path, "many_lights", size=(24, 16))
    check(hs2, dev2)
