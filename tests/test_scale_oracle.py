"""The scaled, shifted and far-viewed inputs of tests/scale_scenes.py, checked with the CPU oracle
alone: its two traversal modes (reference fp64 slabs; the device's conservative fp32 boxes grown by
delta = 2^-20 max|vertex|) give the same pixels and ray counts, the oracle equals minirt's brute
force where that is affordable, and the inputs are not vacuous.  tests/test_scale_gpu.py compares
the device with the oracle on exactly these inputs and relies on what this file asserts."""
import ctypes as C

import numpy as np
import pytest

import query_cases as qc
import rtamd
import scale_scenes as ss
from rtamd import abi

REF, ORD = ss.REF, ss.ORD


def _same_in_both_modes(key, spp):
    img, cnt = ss.frame(key, spp, REF)
    img2, cnt2 = ss.frame(key, spp, ORD)
    assert np.array_equal(img, img2), float(np.abs(img - img2).max())
    assert ss.rays_counted(cnt) == ss.rays_counted(cnt2)
    assert int(cnt.closest_hits) == int(cnt2.closest_hits)
    return cnt


@pytest.mark.parametrize("seed", ss.SEEDS)
@pytest.mark.parametrize("tname", sorted(ss.TRANSFORMS))
def test_reference_and_ordered_modes_agree(tname, seed):
    cnt = _same_in_both_modes(ss.fuzz_key(tname, seed), ss.spp_of(seed))
    assert cnt.primary_rays == ss.W * ss.H * ss.spp_of(seed) ** 2


@pytest.mark.parametrize("tname", sorted(ss.TRANSFORMS))
def test_inputs_are_not_vacuous(tname):
    ss.check_not_vacuous(tname)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("tname", sorted(ss.TRANSFORMS))
def test_conservative_boxes_lose_no_hit(tname, seed):
    # What delta is for: every hit the fp64 triangle test accepts survives the fp32 boxes.  Rays
    # aimed at mesh vertices run along the corners of the leaf boxes, where a growth that does not
    # scale with max|vertex| loses hits first; random rays beside them.  The reference is the
    # triangle test over all triangles with no hierarchy; t is compared bit for bit.
    hs, orc = ss.case(ss.fuzz_key(tname, seed))
    P = hs.soa_arrays()["vertex_pos"]
    rays = np.concatenate([qc.vertex_rays(hs, P, 256, seed=5 + seed), qc.random_rays(hs, 128, seed=7 + seed)])
    want = ss.brute_force_t(hs, rays)
    got = qc.oracle_hits(orc, rays, ORD)
    assert np.array_equal(got["t"], want), int((got["t"] != want).sum())
    # of 384 rays (|S| < 1e-10 rejects ordinary triangles at 2^-16 and all of them at 2^-20)
    n_hit = int(np.isfinite(want).sum())
    assert n_hit >= {ss.ALL_REJECTED: 0, ss.PARTLY_REJECTED: 32}.get(tname, 96), n_hit
    assert n_hit == 0 or tname != ss.ALL_REJECTED


def _matches_brute_force(key, defn, spp):
    # pixels within 1e-12 and ray counts exact, as tests/test_fuzz_oracle.py compares the two
    img, cnt = ss.frame(key, spp, REF)
    mini = ss.mini(defn)
    ref = np.array(mini.render(spp))
    assert img.shape == ref.shape
    assert np.abs(img - ref).max() <= 1e-12, np.abs(img - ref).max()
    assert ss.rays_counted(cnt) == [mini.counts["primary"], mini.counts["shadow"], mini.counts["reflection"]]
    _same_in_both_modes(key, spp)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("tname", ss.BRUTE_TRANSFORMS)
def test_fuzz_scene_matches_brute_force(tname, seed):
    s, t = ss.TRANSFORMS[tname]
    _matches_brute_force(ss.fuzz_key(tname, seed, 9, 7), ss.transformed(seed, s, t, 9, 7), ss.spp_of(seed))


@pytest.mark.parametrize("name", ss.KAT_NAMES)
@pytest.mark.parametrize("tname", ss.BRUTE_TRANSFORMS)
def test_kat_scene_matches_brute_force(tname, name):
    s, t = ss.TRANSFORMS[tname]
    _matches_brute_force(("kat", tname, name), ss.transformed_kat(name, s, t), 1)


@pytest.mark.parametrize("seed", ss.VARIANT_SEEDS)
@pytest.mark.parametrize("vname", sorted({**ss.VARIANTS, **ss.CPU_ONLY_VARIANTS}))
def test_variants_agree_in_both_modes(vname, seed):
    cnt = _same_in_both_modes(("variant", vname, seed), 1)
    assert cnt.closest_hits > 0


def test_variants_move_what_they_say():
    hs0, _ = ss.case(ss.fuzz_key("identity", 0))
    lo, hi = qc.root_box(hs0)
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    centre = 0.5 * (lo + hi)
    raw0 = hs0.raw.contents
    hs, _ = ss.case(("variant", "sun1e6", 0))
    raw = hs.raw.contents
    far = np.array(raw.lights[0].position[:]) - centre
    assert abs(np.sqrt((far * far).sum()) / diag - 1e6) < 1.0
    assert raw.n_lights == raw0.n_lights
    hs, _ = ss.case(("variant", "telephoto1e4", 0))
    back = np.array(hs.raw.contents.camera.eye[:]) - np.array(raw0.camera.eye[:])
    assert abs(np.sqrt((back * back).sum()) / diag - 1e4) < 1e-6
    # the image plane is the one the unit camera has: same pixel vectors to rounding
    c0, c1 = hs0.camera(), hs.camera()
    assert np.allclose(c1.x_dir[:], c0.x_dir[:], rtol=1e-9, atol=0.0)
    assert np.allclose(c1.lower_left[:], c0.lower_left[:], rtol=1e-6, atol=1e-9)
    hs, _ = ss.case(("variant", "outlier1e12", 0))
    assert qc.root_box(hs)[1][0] == 1e12


@pytest.mark.parametrize("factor", ss.FAR_FACTORS)
@pytest.mark.parametrize("flavour", ss.FAR_FLAVOURS)
@pytest.mark.parametrize("name", ss.FAR_SCENES)
def test_far_rays_agree_in_both_modes(name, flavour, factor):
    hs, orc, _, _, _ = ss.far_scene(name)
    rays, want = ss.far_case(name, flavour, factor)
    assert len(rays) == 256
    ref = qc.oracle_hits(orc, rays, REF)
    for k in ("hit", "t", "tri", "normal", "point"):
        assert np.array_equal(ref[k], want[k]), k
    # the set means something: rays that hit and, with a finite tmax, hits on both sides of it
    assert want["hit"].sum() >= 64
    if flavour == "axis":
        assert np.all((rays[:, 3:6] == 0.0).sum(axis=1) == 2)
    if flavour == "tmax":
        cut = ss.within_tmax(want, rays)["hit"]
        assert cut.any() and (want["hit"] & ~cut).any()
        assert np.all(np.isfinite(rays[:, 6]))
    lo, hi = qc.root_box(hs)
    away = np.sqrt(((rays[:, 0:3] - 0.5 * (lo + hi)) ** 2).sum(axis=1)) / np.sqrt(((hi - lo) ** 2).sum())
    assert np.all(away > factor - 1.0) and np.all(away < factor + 1.0)


# ---- the supported coordinate range (rt_hip.h at rt_scene_upload) ----
def _upload_code(hs):
    """The code rt_scene_upload would return for a prepared scene (rt_debug_tree_report: no device)."""
    opt = rtamd.upload_options()
    rep = abi.TreeReport()
    return int(rtamd.hip_lib().rt_debug_tree_report(hs.soa, hs.bvh, C.byref(opt), C.byref(rep)))


def test_coordinates_beyond_the_supported_range_are_refused():
    # the oracle handles them (its ordered mode has no fused slab) ...
    _same_in_both_modes(("scaled", 1e20, 0), 1)
    _same_in_both_modes(("scaled", ss.TOP_SCALE, 0), 1)
    # ... upload refuses them, and takes everything this module renders otherwise
    for key in (("variant", "outlier1e30", 0), ("variant", "outlier1e30", 1), ("scaled", 1e20, 0)):
        assert _upload_code(ss.case(key)[0]) == abi.RT_ERR_UNSUPPORTED, key
    for key in (ss.fuzz_key("x2^20", 0), ss.fuzz_key("x2^-20", 0), ("variant", "outlier1e12", 0),
                ("variant", "outlier2^61", 0), ("scaled", ss.TOP_SCALE, 0)):
        assert _upload_code(ss.case(key)[0]) == abi.RT_OK, key
    assert abi.RT_MAX_COORDINATE == 2.0 ** 61
    assert qc.root_box(ss.case(("variant", "outlier2^61", 0))[0])[1][0] == abi.RT_MAX_COORDINATE
